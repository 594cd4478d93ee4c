"""The MLA sparse indexer (fa_mi355x.flash_attention_mla_indexer*) on the GPU:
the index logits against the float64 evaluation of
include/fa_mi355x_mla_indexer.h's contract on the same rounded inputs, the
selection against torch.sort on the logits the test supplies (exact), the
composition, and rows past 4 GiB.

Logits gate, per element: 2^-23 * 192 * A[n][j], A = k_scale * sum_h |w| *
sum_d |q k| in float64: the forward bound of 192 sequential fp32 operations
(128 of the dot product, 64 of the head sum) of unit roundoff 2^-24, doubled;
the bound passes through the 1-Lipschitz ReLU.  test_gate_is_sharp (no GPU)
shows a plain fp32 evaluation within half of it and the gate below a 64th
of the logits' spread, one head's share."""
import functools

import pytest
import torch

import decode_refs as dr
import fa_mi355x as fa

gpu = pytest.mark.gpu
DEV = dr.DEV
H, D, R, MAX_LEN, SENTINEL = 64, 128, 1000, 256, -12345.0
# nine tokens (a ragged third block of four), ks no multiple of 64, neighbours disjoint: lengths 0, 1, 63,
# 64, 65, 200, an inverted range, ke past the pool (30 rows left), a length above max_len (300 -> 256)
KS = [5, 7, 70, 133, 300, 401, 650, 970, 601]
KE = [5, 8, 133, 197, 365, 601, 640, R + 50, 901]
LENS = [0, 1, 63, 64, 65, 200, 0, 30, 256]
N = len(KS)
KINDS = [pytest.param(False, id="k16"), pytest.param(True, id="k8")]


@functools.lru_cache(maxsize=None)
def host_inputs(dtype, k8):
    """q, k (rounded to their types), weights of both signs, k_scale in [0.5, 2), the float64 reference
    [N, MAX_LEN] and its gate; every pool row outside all ranges is NaN (byte 0x7f for k8)."""
    gen = torch.Generator().manual_seed(11 + k8)
    q = (torch.rand((N, H, D), generator=gen) * 2 - 1).to(dtype)
    k = torch.rand((R, D), generator=gen) * 2 - 1
    k = k.to(torch.float8_e4m3fn) if k8 else k.to(dtype)
    w = torch.rand((N, H), generator=gen) * 2 - 1
    scale = torch.rand(R, generator=gen) * 1.5 + 0.5 if k8 else torch.ones(R)
    used = torch.zeros(R, dtype=torch.bool)
    for s, n in zip(KS, LENS):
        used[s:s + n] = True
    q64, k64, w64 = q.double(), k.float().double(), w.double()
    ref, gate = torch.zeros((N, MAX_LEN), dtype=torch.float64), torch.zeros((N, MAX_LEN), dtype=torch.float64)
    for n, (s, ln) in enumerate(zip(KS, LENS)):
        kk, sc = k64[s:s + ln], scale[s:s + ln].double()
        ref[n, :ln] = sc * (w64[n, :, None] * torch.relu(q64[n] @ kk.T)).sum(0)
        gate[n, :ln] = 2.0 ** -23 * 192 * sc * (w64[n].abs()[:, None] * (q64[n].abs() @ kk.abs().T)).sum(0)
    if k8:
        k.view(torch.uint8)[~used] = 0x7f
    else:
        k.view(torch.int16)[~used] = dr.NAN_BITS
    return q, k, w, scale, ref, gate


def device_args(dtype, k8, n=N):
    q, k, w, scale, _, _ = host_inputs(dtype, k8)
    rng = [torch.tensor(x[:n], dtype=torch.int32, device=DEV) for x in (KS, KE)]
    return (q[:n].to(DEV), k.to(DEV), w[:n].to(DEV), *rng), dict(k_scale=scale.to(DEV)) if k8 else {}


def check_logits(out, dtype, k8):
    _, _, _, _, ref, gate = host_inputs(dtype, k8)
    out = out.cpu()
    for n, ln in enumerate(LENS):
        err = (out[n, :ln].double() - ref[n, :ln]).abs()
        assert bool((err <= gate[n, :ln]).all()), (n, float((err / gate[n, :ln]).max()))
        assert bool((out[n, ln:] == SENTINEL).all()), n  # columns past the length are not written


@pytest.mark.parametrize("k8", KINDS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_gate_is_sharp(dtype, k8):
    q, k, w, scale, ref, gate = host_inputs(dtype, k8)
    live = []
    for n, (s, ln) in enumerate(zip(KS, LENS)):
        got = scale[s:s + ln] * (w[n, :, None] * torch.relu(q[n].float() @ k[s:s + ln].float().T)).sum(0)
        assert bool(((got.double() - ref[n, :ln]).abs() <= gate[n, :ln] / 2).all()), n
        live.append(ref[n, :ln])
    # a lost or wrongly weighted head moves a logit by about 1/64 of the logits' spread
    assert float(gate.max()) < float(torch.cat(live).std()) / 64


@gpu
@pytest.mark.parametrize("k8", KINDS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_logits_match_float64(dtype, k8):
    args, kw = device_args(dtype, k8)
    out = torch.full((N, MAX_LEN), SENTINEL, device=DEV)
    assert fa.flash_attention_mla_indexer_logits(*args, out=out, **kw) is out
    check_logits(out, dtype, k8)
    again = torch.full((N, MAX_LEN + 7), SENTINEL, device=DEV)  # a row stride above max_len; the same bits
    fa.flash_attention_mla_indexer_logits(*args, out=again, max_len=MAX_LEN, **kw)
    assert torch.equal(again[:, :MAX_LEN], out) and bool((again[:, MAX_LEN:] == SENTINEL).all())


@gpu
@pytest.mark.parametrize("k8", KINDS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_census(dtype, k8):
    """q = k = 1/8 and weights 1: every logit is exactly 128; half the weights -1: exactly 0."""
    n, rows = 5, 300
    q = torch.full((n, H, D), 0.125, dtype=dtype, device=DEV)
    k = torch.full((rows, D), 0.125, device=DEV).to(torch.float8_e4m3fn if k8 else dtype)
    kw = dict(k_scale=torch.ones(rows, device=DEV)) if k8 else {}
    ks = torch.tensor([0, 3, 64, 100, 299], dtype=torch.int32, device=DEV)
    ke = torch.tensor([300, 67, 128, 101, 300], dtype=torch.int32, device=DEV)
    for sign, want in ((1.0, 128.0), (-1.0, 0.0)):
        w = torch.ones((n, H), device=DEV)
        w[:, 1::2] = sign
        out = fa.flash_attention_mla_indexer_logits(q, k, w, ks, ke, out=torch.full((n, rows), SENTINEL, device=DEV), **kw)
        cols = torch.arange(rows, device=DEV)[None, :] < (ke - ks)[:, None]
        assert bool((out == torch.where(cols, want, SENTINEL)).all()), sign


VALUES = ["normal", "ints", "equal", "zeros", "inf"]
WIDTH = 5000


@functools.lru_cache(maxsize=None)
def select_case(topk, values):
    """logits [6, 5000] on the CPU, ks, ke (lengths 0, 1, topk - 1, topk, topk + 1, 5000; ks > 0) and the
    expected lists: a stable descending torch.sort, the kept columns sorted, + ks, padded with -1."""
    gen = torch.Generator().manual_seed(topk + VALUES.index(values))
    x = torch.randn((6, WIDTH), generator=gen)
    if values == "ints":
        x = torch.randint(0, 8, (6, WIDTH), generator=gen).float()  # hundreds of ties in the threshold bucket
    elif values == "equal":
        x = torch.full((6, WIDTH), -2.5)
    elif values == "zeros":
        x = torch.where(x > 0.5, x, torch.where(x > 0, 0.0, -0.0))  # +0 and -0 are one value
    elif values == "inf":
        x = torch.where(x < 0, -float("inf"), x)
    lens = [0, 1, topk - 1, topk, topk + 1, WIDTH]
    ks = [17 * (n + 1) for n in range(6)]
    want = torch.full((6, topk), -1, dtype=torch.int32)
    for n, ln in enumerate(lens):
        keep = torch.sort(x[n, :ln], stable=True, descending=True).indices[:topk].sort().values
        want[n, :len(keep)] = keep.int() + ks[n]
    return x, ks, [s + ln for s, ln in zip(ks, lens)], want


@gpu
@pytest.mark.parametrize("stride,values", [(WIDTH, v) for v in VALUES] + [(WIDTH + 3, "ints")])
@pytest.mark.parametrize("topk", [1, 64, 2048])
def test_selection_matches_sort(topk, stride, values):
    x, ks, ke, want = select_case(topk, values)
    buf = torch.full((6, stride), float("nan"), device=DEV)
    buf[:, :WIDTH] = x.to(DEV)
    ks, ke = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (ks, ke))
    got = fa.flash_attention_mla_indexer_topk(buf[:, :WIDTH], ks, ke, topk, num_rows=6000)
    assert torch.equal(got.cpu(), want)


@gpu
@pytest.mark.parametrize("k8", KINDS)
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_composition(dtype, k8):
    import fa_mi355x.torch_op_mla_indexer as top

    args, kw = device_args(dtype, k8)
    scale = kw.get("k_scale")
    logits = fa.flash_attention_mla_indexer_logits(*args, max_len=MAX_LEN, **kw)
    lists = fa.flash_attention_mla_indexer_topk(logits, args[3], args[4], 48, num_rows=R)
    for n, (s, ln) in enumerate(zip(KS, LENS)):
        row = lists[n].cpu()
        assert int((row >= 0).sum()) == min(48, ln) and bool(((row == -1) | ((row >= s) & (row < s + ln))).all()), n
    for _ in range(2):  # the pair in one call, twice: the same bits
        assert torch.equal(fa.flash_attention_mla_indexer(*args, topk=48, max_len=MAX_LEN, **kw), lists)
    for n, ln in enumerate(LENS):
        assert torch.equal(top.indexer_logits(*args, MAX_LEN, scale)[n, :ln], logits[n, :ln]), n
    assert torch.equal(top.indexer_topk(logits, args[3], args[4], 48, R), lists)
    assert torch.equal(top.indexer(*args, 48, MAX_LEN, scale), lists)


@gpu
def test_logits_row_past_4gib():
    """N = 2 with a row stride of 2^30 + 64 elements: token 1's row starts past 4 GiB."""
    args, _ = device_args(torch.float16, False, n=2)
    args = list(args)
    args[3], args[4] = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([401, 70], [601, 133]))
    want = fa.flash_attention_mla_indexer_logits(*args, max_len=MAX_LEN)
    stride = 2 ** 30 + 64
    view = torch.empty(2 * stride, device=DEV).as_strided((2, MAX_LEN), (stride, 1))
    view.fill_(SENTINEL)
    fa.flash_attention_mla_indexer_logits(*args, out=view)
    for n, ln in enumerate((200, 63)):
        assert torch.equal(view[n, :ln], want[n, :ln]) and bool((view[n, ln:] == SENTINEL).all()), n
    lists = fa.flash_attention_mla_indexer_topk(view, args[3], args[4], 16, num_rows=R)
    assert torch.equal(lists, fa.flash_attention_mla_indexer_topk(want, args[3], args[4], 16, num_rows=R))


@gpu
def test_key_rows_past_4gib():
    """A pool of 2^24 + 256 rows (256 B each): the ranged rows lie past 4 GiB; nothing else is initialised."""
    (q, k, w, _, _), _ = device_args(torch.float16, False, n=2)
    base = 2 ** 24 + 10
    pool = torch.empty((2 ** 24 + 256, D), dtype=torch.float16, device=DEV)
    pool[base:base + 200] = k[401:601]
    ks = torch.tensor([base, base + 100], dtype=torch.int32, device=DEV)
    ke = torch.tensor([base + 200, base + 165], dtype=torch.int32, device=DEV)
    got = fa.flash_attention_mla_indexer_logits(q, pool, w, ks, ke, out=torch.full((2, MAX_LEN), SENTINEL, device=DEV))
    want = fa.flash_attention_mla_indexer_logits(q, k, w, ks - base + 401, ke - base + 401, max_len=MAX_LEN)
    for n, ln in enumerate((200, 65)):
        assert torch.equal(got[n, :ln], want[n, :ln]) and bool((got[n, ln:] == SENTINEL).all()), n
