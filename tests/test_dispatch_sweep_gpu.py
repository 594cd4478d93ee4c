"""Dispatcher-level sweep: random and tier-boundary shapes through both entry
points a caller has -- the Python/torch path (`flash_attention_fwd`, which
brings the workspace: causal split tier, W4 tail pool) and the
workspace-free C entry (`fa_fwd_f16` / `fa_fwd_bf16`, what the reference's
`flash_attention_v9_dispatch` signature reaches, flash_attention.cu:606-611)
-- against an fp32 torch attention of the same 16-bit inputs.

The per-tier tests force one config each; this file checks that the
dispatcher's choice (`fa_select_config`, the split / pool / W4P / W4 /
KV-pair / KV-quad / loop boundaries in fa_fwd.hip) is right wherever it
lands: every shape must match at 1e-3 (fp16) or 2.5e-3 (bf16), whichever
tier runs it.  Since round 6 every bf16 tier scales the fp32 scores by
log2(e)/sqrt(d) instead of feeding a bf16-rounded Q * scale to the MFMA, so
bf16 is gated against the plain fp32 model on peaked inputs too (round 5:
5e-3 against a model with that rounding, 1e-2 against the plain one).
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from fwd_helpers import BOUNDARY, fa as _fa, ref_fp32_by_head as _ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _random_shapes(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        b = int(rng.integers(1, 5))
        h = int(rng.integers(1, 41))
        s = int(round(math.exp(rng.uniform(0.0, math.log(5000)))))
        d = int(rng.choice([64, 128]))
        causal = bool(rng.integers(0, 2))
        bf16 = bool(rng.random() < 0.3)
        while b * h * s * s * d > 4e9 and s > 1:
            s //= 2
        out.append((b, h, s, d, causal, bf16))
    return out


def _inputs(b, h, s, d, dtype, seed, scale):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return [torch.empty((b, h, s, d), dtype=torch.float32, device="cuda")
            .uniform_(-0.5 * (scale if i < 2 else 1.0), 0.5 * (scale if i < 2 else 1.0), generator=g)
            .to(dtype) for i in range(3)]


def _run(shape, seed, scale=1.0):
    fa = _fa()
    b, h, s, d, causal, bf16 = shape
    dtype = torch.bfloat16 if bf16 else torch.float16
    # bf16: P and O round to 8 significant bits (O on [-0.5, 0.5]: half an
    # ulp is ~1e-3); the scores stay fp32 (round 5's bf16 Q * scale gave
    # 4.3-5.2e-3 on peaked inputs, profiles/r05_bf16_peaked_err.jsonl)
    tol = 2.5e-3 if bf16 else 1e-3
    q, k, v = _inputs(b, h, s, d, dtype, seed, scale)
    ref = _ref(q, k, v, causal)
    # the Python / torch path: workspace entry
    o1 = fa.flash_attention_fwd(q, k, v, causal)
    torch.cuda.synchronize()
    err1 = (o1.float() - ref).abs().max().item()
    # the workspace-free C entry (the reference signature's path)
    o2 = torch.full_like(q, float("nan"))
    lib = fa.load_library()
    fn = lib.fa_fwd_bf16 if bf16 else lib.fa_fwd_f16
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o2.data_ptr(), b, h, s, d, int(causal),
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fa_status_string(rc)
    torch.cuda.synchronize()
    err2 = (o2.float() - ref).abs().max().item()
    cfg = fa.configs()[fa.select_config(b, h, s, causal)].name if d == 128 and not bf16 else "-"
    assert err1 <= tol and err2 <= tol, (shape, cfg, err1, err2)


@pytest.mark.parametrize("shape", _random_shapes(40, 2028), ids=lambda s: "x".join(map(str, s)))
def test_dispatch_random(shape):
    _run(shape, 11)


@pytest.mark.parametrize("shape", BOUNDARY, ids=lambda s: "x".join(map(str, s)))
def test_dispatch_boundary(shape):
    _run(shape, 23)


@pytest.mark.parametrize("shape", BOUNDARY, ids=lambda s: "x".join(map(str, s)))
def test_dispatch_boundary_peaked(shape):
    """q, k on [-3, 3]: scores spread over tens of log2 units, so every
    tier's lazy rescale (m_ref moves past 8) runs mid-row"""
    _run(shape, 37, scale=6.0)
