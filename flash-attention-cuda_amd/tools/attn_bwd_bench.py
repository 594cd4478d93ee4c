#!/usr/bin/env python3
"""Benchmark of the attention backward pass (flash_attention_varlen_backward:
the delta, dK/dV and dQ kernels of csrc/fa_attn_bwd_kernel.hpp) at D = 128,
Hq = 32, Hkv = 8, on the --selfattn batches of tools/prefill_bench.py:

  uniform   8 prompts of 4096 tokens, causal;
  ragged    prompts of 512, 1024, ... 4096 tokens, causal;
  vit       32 non-causal ViT-like images.

One invocation = one batch and one dtype (run it under `timeout`), one JSON line.
Arms, alternated round by round after a warm-up (prefill_bench.py's loop):

  fwd    flash_attention_varlen with return_lse (what the backward recomputes from);
  bwd    the backward: three launches on out, lse and a fixed dout;
  sdpa   torch.nn.functional.scaled_dot_product_attention's backward alone
         (torch.autograd.grad on a retained graph, sequence by sequence, [1, H,
         n, D] with enable_gqa), whatever backend torch picks on the box;
  bwd2   `bwd` again: bwd_aa is the spread of the box.

Reported: the arms' times, bwd_over_fwd, bwd TFLOP/s by 10 Hq D sum n^2 (halved
under causal), sdpa_over_bwd (> 1: torch is slower), and the three kernels'
own times from torch.profiler (null where the profiler gives no kernel events).
Nothing is gated on these numbers.

    timeout 600 python3 tools/attn_bwd_bench.py --batch uniform --dtype bf16 [--out profiles/attn_bwd_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fa_mi355x  # noqa: E402
from prefill_bench import SELFATTN, selfattn_lengths, time_arms  # noqa: E402

KERNELS = ("delta", "dkdv", "dq")


def kernel_times(fn, calls):
    """Mean ms per call of each of the three kernels, by torch.profiler; None
    for a kernel the profiler shows no event of."""
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = dict.fromkeys(KERNELS)
        for ev in prof.key_averages():
            for name in KERNELS:
                if "fa_attn_bwd_%s_kernel" % name in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = ev.cuda_time_total
                    out[name] = (out[name] or 0.0) + us / 1e3 / calls
        return out
    except Exception as e:  # the tool reports it; the arms' own times do not depend on it
        return {"error": "%s: %s" % (type(e).__name__, e)}


def run(name, dt, rounds, iters, with_sdpa):
    n, causal = selfattn_lengths(name)
    b, hq, hkv, d = len(n), 32, 8, 128
    total = sum(n)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    q, k, v, do = rnd(total, hq, d), rnd(total, hkv, d), rnd(total, hkv, d), rnd(total, hq, d)
    cu_host = [0] + [sum(n[:i + 1]) for i in range(b)]
    cu = torch.tensor(cu_host, dtype=torch.int32, device="cuda")
    out, lse = fa_mi355x.flash_attention_varlen(q, k, v, cu, causal=causal, return_lse=True)
    grads = [torch.empty_like(t) for t in (q, k, v)]

    def fwd():
        return fa_mi355x.flash_attention_varlen(q, k, v, cu, causal=causal, out=out, return_lse=True)

    def bwd():
        return fa_mi355x.flash_attention_varlen_backward(do, q, k, v, out, lse, cu, causal=causal, dq=grads[0],
                                                         dk=grads[1], dv=grads[2])

    arms, names = [fwd, bwd], ["fwd", "bwd"]
    rec = dict(batch_name=name, dtype=str(dt).split(".")[-1], causal=causal, batch=b, heads_q=hq, heads_kv=hkv,
               head_dim=d, total=total, max_n=max(n), rounds=rounds, iters=iters)
    if with_sdpa:
        try:
            graphs = []
            for s, e in zip(cu_host[:-1], cu_host[1:]):
                qs, ks, vs = (t[s:e].transpose(0, 1)[None].detach().requires_grad_() for t in (q, k, v))
                o = F.scaled_dot_product_attention(qs, ks, vs, is_causal=causal, enable_gqa=True)
                graphs.append((o, (qs, ks, vs), do[s:e].transpose(0, 1)[None]))

            def sdpa():
                return [torch.autograd.grad(o, leaves, g, retain_graph=True) for o, leaves, g in graphs]

            got = sdpa()
            bwd()
            rec["max_abs_diff_dq_vs_sdpa"] = max(
                float((g[0][0].transpose(0, 1).float() - grads[0][s:e].float()).abs().max())
                for g, s, e in zip(got, cu_host[:-1], cu_host[1:]))
            del got
            arms.append(sdpa)
            names.append("sdpa")
        except Exception as e:
            rec["sdpa_error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
    arms.append(bwd)
    names.append("bwd2")
    ts = dict(zip(names, time_arms(arms, iters, rounds)))
    for arm, (med, lo, hi) in ts.items():
        rec[arm + "_ms"] = round(med, 4)
        rec[arm + "_min_ms"] = round(lo, 4)
        rec[arm + "_max_ms"] = round(hi, 4)
    fl = 10.0 * hq * d * sum(x * x for x in n) * (0.5 if causal else 1.0)
    rec["bwd_tflops"] = round(fl / (ts["bwd"][0] * 1e-3) / 1e12, 1)
    rec["fwd_tflops"] = round(0.4 * fl / (ts["fwd"][0] * 1e-3) / 1e12, 1)
    rec["bwd_over_fwd"] = round(ts["bwd"][0] / ts["fwd"][0], 4)
    rec["bwd_aa"] = round(ts["bwd2"][0] / ts["bwd"][0], 4)
    if "sdpa" in ts:
        rec["sdpa_over_bwd"] = round(ts["sdpa"][0] / ts["bwd"][0], 4)
    kt = kernel_times(bwd, 5)
    rec["kernel_ms"] = {key: (round(val, 4) if isinstance(val, float) else val) for key, val in kt.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", choices=SELFATTN, required=True)
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--no-sdpa", action="store_true", help="skip the torch SDPA backward arm")
    ap.add_argument("--out", default=None, help="appended to; default profiles/attn_bwd_bench.jsonl")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attn_bwd_bench.py needs a GPU")
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles",
                                "attn_bwd_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    rec = run(args.batch, dt, args.rounds, args.iters, not args.no_sdpa)
    rec["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
