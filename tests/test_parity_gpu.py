"""GPU parity: the HIP forward path (through the C ABI) vs the CPU oracle.

Gate: max-abs fp16 difference <= 1e-3 (BASELINE.json north_star), i.e. 100x
tighter than the reference's own 0.1 threshold (flash_attention.cu:784).
Inputs: the reference generator (srand(42), uniform [-0.5, 0.5] -> fp16,
flash_attention.cu:764-769) unless a test says otherwise.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import oracle  # noqa: E402  (test infrastructure)
from fwd_helpers import fa as _fa, to_dev as _to_dev, to_host_bits as _to_host_bits  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-3


def _run(q, k, v, causal, config=None, splitkv=False, num_splits=0):
    fa = _fa()
    dq, dk, dv = _to_dev(q), _to_dev(k), _to_dev(v)
    if splitkv:
        o = fa.flash_attention_fwd_splitkv(dq, dk, dv, causal=causal, num_splits=num_splits)
    else:
        o = fa.flash_attention_fwd(dq, dk, dv, causal=causal, config=config)
    torch.cuda.synchronize()
    return _to_host_bits(o)


_cache = {}


def _case(b, h, s, causal, seed=42, qk_scale=1.0):
    key = (b, h, s, causal, seed, qk_scale)
    if key not in _cache:
        q, k, v = oracle.gen_inputs(b, h, s, 128, seed)
        if qk_scale != 1.0:
            # peaked softmax: scale Q and K in fp16 (exact for powers of two)
            f = lambda a: (oracle.f16_bits_to_f32(a) * qk_scale).astype(np.float16).view(np.uint16)
            q, k = f(q), f(k)
        ref = oracle.attention(q, k, v, causal)
        _cache[key] = (q, k, v, ref)
    return _cache[key]


# --- the reference's four correctness checks (flash_attention.cu:757-884) ----
@pytest.mark.parametrize(
    "s,h,causal",
    [(256, 32, True), (1024, 32, True), (1024, 32, False), (2048, 2, False)],
    ids=["s256_h32_causal", "s1024_h32_causal", "s1024_h32_noncausal", "s2048_h2_noncausal"],
)
def test_reference_checks(s, h, causal):
    q, k, v, ref = _case(1, h, s, causal)
    out = _run(q, k, v, causal)
    d = oracle.max_abs_diff(out, ref)
    assert d <= TOL, f"max_diff={d}"


# --- every tile config, both masks, incl. the causal-long tier the reference never checks
def _configs(causal, split=False):
    fa = _fa()
    return [c.id for c in fa.configs()
            if c.causal == causal and c.split_kv == split and c.dtype == "float16"
            and c.head_dim == 128]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("s", [512, 2048])
def test_every_config(causal, s):
    q, k, v, ref = _case(1, 4, s, causal)
    for cid in _configs(causal):
        out = _run(q, k, v, causal, config=cid)
        d = oracle.max_abs_diff(out, ref)
        assert d <= TOL, f"config {cid}: max_diff={d}"


# --- ragged sequence lengths (not a multiple of any tile) ----------------------
@pytest.mark.parametrize("s", [1, 7, 77, 129, 300, 1000])
@pytest.mark.parametrize("causal", [False, True])
def test_ragged(s, causal):
    q, k, v, ref = _case(2, 3, s, causal, seed=7)
    for cid in _configs(causal):
        out = _run(q, k, v, causal, config=cid)
        d = oracle.max_abs_diff(out, ref)
        assert d <= TOL, f"s={s} config {cid}: max_diff={d}"


# --- peaked softmax (Q,K x4): exercises the lazy-rescale branch ------------------
@pytest.mark.parametrize("causal", [False, True])
def test_peaked_softmax(causal):
    q, k, v, ref = _case(1, 4, 1024, causal, seed=3, qk_scale=4.0)
    for cid in _configs(causal):
        out = _run(q, k, v, causal, config=cid)
        d = oracle.max_abs_diff(out, ref)
        assert d <= TOL, f"config {cid}: max_diff={d}"


# --- batch > 1 ------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_batch(causal):
    q, k, v, ref = _case(3, 5, 384, causal, seed=11)
    out = _run(q, k, v, causal)
    assert oracle.max_abs_diff(out, ref) <= TOL


# --- split-KV + LSE merge --------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("num_splits", [0, 1, 3, 8])
def test_splitkv(causal, num_splits):
    q, k, v, ref = _case(1, 4, 1000, causal, seed=5)
    out = _run(q, k, v, causal, splitkv=True, num_splits=num_splits)
    d = oracle.max_abs_diff(out, ref)
    assert d <= TOL, f"max_diff={d}"


def test_reference_signature_wrapper():
    """flash_attention_v9_dispatch mirror (ref :606-611) with nullptr split buffers."""
    fa = _fa()
    q, k, v, ref = _case(1, 32, 256, True)
    dq, dk, dv = _to_dev(q), _to_dev(k), _to_dev(v)
    o = torch.empty_like(dq)
    fa.flash_attention_v9_dispatch(dq, dk, dv, o, None, None, 1, 32, 256, 128, True)
    torch.cuda.synchronize()
    assert oracle.max_abs_diff(_to_host_bits(o), ref) <= TOL


def test_error_codes():
    fa = _fa()
    q = torch.zeros(1, 1, 64, 96, dtype=torch.float16, device="cuda")  # head_dim 64/128 only
    with pytest.raises(fa.FlashAttentionError) as e:
        fa.flash_attention_v9_dispatch(q, q, q, q, None, None, 1, 1, 64, 96, False)
    assert e.value.status == fa.FA_ERR_UNSUPPORTED_HEAD_DIM


@pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2,
                    reason="needs two GPUs")
def test_non_current_device():
    """Tensors on cuda:1 while cuda:0 is current: the launch goes to cuda:1
    (the C side sizes and launches on the current device, so the binding
    switches to q's device); tensors split over devices are rejected."""
    fa = _fa()
    q, k, v, ref = _case(1, 4, 256, True)
    torch.cuda.set_device(0)
    d1 = torch.device("cuda", 1)
    dq, dk, dv = (torch.from_numpy(a.view(np.int16)).view(torch.float16).to(d1) for a in (q, k, v))
    o = fa.flash_attention_fwd(dq, dk, dv, causal=True)
    torch.cuda.synchronize(d1)
    assert o.device == d1
    assert oracle.max_abs_diff(_to_host_bits(o), ref) <= TOL
    with pytest.raises(fa.FlashAttentionError):
        fa.flash_attention_fwd(dq, dk.to("cuda:0"), dv, causal=True)
