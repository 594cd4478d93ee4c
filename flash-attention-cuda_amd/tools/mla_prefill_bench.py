#!/usr/bin/env python3
"""MLA prefill benchmark: fa_mi355x.flash_attention_mla_prefill_varlen (192-dim
Q/K, 128-dim V) against what a caller runs for these dims without it and
against this library's own D = 128 attention, alternated in one process by
tools/decode_bench.py's method: kernel / SDPA / kernel / D = 128 round by
round, so every row carries its own A/A spread (aa, the second kernel leg over
the first) beside sdpa_over_kernel and the two rates.

  arm 1  the new entry;
  arm 2  torch.nn.functional.scaled_dot_product_attention on [B, H, S, 192]
         with scale=, restricted to the fused backends (the math backend would
         materialise the scores); where it refuses the 128-dim V, V is padded
         to 192 (`sdpa` records which: "v128", "v192" or "refused").  A ragged
         batch is one call per sequence;
  arm 3  flash_attention_varlen at D = 128 on the same tokens: the yardstick
         for rate per FLOP, not a competitor (it computes another function).

Shapes at Hq = Hkv = 16 and 128, fp16 and bf16: 8 x 4096 causal, one 32k
prompt causal, a ragged batch 512 .. 4096 causal, and the chunked-prefill
context call (a 256-row chunk against 32k keys, non-causal).  FLOPs are
2 * (192 + 128) per visible (row, key) pair (arm 3: 2 * 256).

    python3 tools/mla_prefill_bench.py [--out profiles/mla_prefill_bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch.nn.attention import SDPBackend, sdpa_kernel

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402
from decode_bench import time_pair  # noqa: E402

DQK, DV = 192, 128
SHAPES = [("8x4096 causal", (4096,) * 8, (4096,) * 8, True),
          ("1x32768 causal", (32768,), (32768,), True),
          ("ragged 512..4096 causal", tuple(range(512, 4097, 512)), tuple(range(512, 4097, 512)), True),
          ("context 256 x 32768 full", (256,), (32768,), False)]


def pairs(nq, nk, causal):
    """Visible (row, key) pairs per head (bottom-right causal)."""
    return sum(sum(max(0, min(k, k - q + i + 1)) for i in range(q)) if causal else q * k for q, k in zip(nq, nk))


def run(name, nq, nk, causal, h, dtype, rounds=5):
    dev, scale = "cuda", DQK ** -0.5
    gen = torch.Generator(device=dev).manual_seed(len(nq) * 131 + h)
    draw = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 2 - 1).to(dtype)
    q, k, v = draw(sum(nq), h, DQK), draw(sum(nk), h, DQK), draw(sum(nk), h, DV)
    cu = lambda n: torch.tensor([0] + list(torch.tensor(n).cumsum(0)), dtype=torch.int32, device=dev)
    cu_q, cu_k = cu(nq), cu(nk)
    q128, k128 = q[..., :DV].contiguous(), k[..., :DV].contiguous()  # arm 3's operands: the first 128 dims
    # arm 2's operands, laid out once outside the timed region: [1, H, S, D] per sequence
    seqs, oq, ok = [], 0, 0
    for a, n in zip(nq, nk):
        seqs.append([t.transpose(0, 1)[None].contiguous() for t in (q[oq:oq + a], k[ok:ok + n], v[ok:ok + n])])
        oq, ok = oq + a, ok + n

    def sdpa(pad):
        outs = []
        with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
            for qs, ks, vs in seqs:
                outs.append(F.scaled_dot_product_attention(qs, ks, F.pad(vs, (0, DQK - DV)) if pad else vs,
                                                           is_causal=causal, scale=scale))
        return outs

    how = "refused"
    for pad, label in ((False, "v128"), (True, "v192")):
        try:
            sdpa(pad)
            torch.cuda.synchronize()
            how, padded = label, pad
            break
        except Exception:  # this backend refuses the shape
            continue
    kernel = lambda i: fa_mi355x.flash_attention_mla_prefill_varlen(q, k, v, cu_q, cu_k, softmax_scale=scale,
                                                                    causal=causal)
    d128 = lambda i: fa_mi355x.flash_attention_varlen(q128, k128, v, cu_q, cu_k, causal=causal)
    fns = [kernel, (lambda i: sdpa(padded)) if how != "refused" else kernel, kernel, d128]
    diff = None
    if how != "refused":
        want = torch.cat([o[0].transpose(0, 1)[..., :DV] for o in sdpa(padded)])
        diff = float((kernel(0).float() - want.float()).abs().max())
    iters = max(1, min(50, int(1e13 / (pairs(nq, nk, causal) * h * 640))))
    t_k, t_s, t_k2, t_d = time_pair(fns, iters, rounds)
    n = pairs(nq, nk, causal) * h
    tf = lambda flops, us: round(flops / (us * 1e-6) / 1e12, 2)
    return dict(name=name, heads=h, dtype=str(dtype).split(".")[-1], iters=iters, kernel_us=round(t_k, 2),
                aa=round(t_k2 / t_k, 4), sdpa=how, sdpa_us=round(t_s, 2) if how != "refused" else None,
                sdpa_over_kernel=round(t_s / t_k, 3) if how != "refused" else None, d128_us=round(t_d, 2),
                kernel_tflops=tf(2.0 * n * (DQK + DV), t_k), d128_tflops=tf(2.0 * n * 2 * DV, t_d),
                rate_over_d128=round((DQK + DV) * t_d / (2 * DV * t_k), 4), max_abs_diff_vs_sdpa=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/mla_prefill_bench.jsonl")
    ap.add_argument("--quick", action="store_true", help="16 heads, bf16 only")
    args = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
    out = args.out or os.path.join(root, "profiles", "mla_prefill_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for dtype in (torch.bfloat16,) if args.quick else (torch.bfloat16, torch.float16):
            for h in (16,) if args.quick else (16, 128):
                for name, nq, nk, causal in SHAPES:
                    rec = run(name, nq, nk, causal, h, dtype)
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
