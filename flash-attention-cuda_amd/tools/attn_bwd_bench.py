#!/usr/bin/env python3
"""Benchmark of the attention backward pass (flash_attention_varlen_backward:
the delta, dK/dV and dQ kernels of csrc/fa_attn_bwd_kernel.hpp) at D = 128,
Hq = 32, Hkv = 8, on the --selfattn batches of tools/prefill_bench.py:

  uniform   8 prompts of 4096 tokens, causal;
  ragged    prompts of 512, 1024, ... 4096 tokens, causal;
  vit       32 non-causal ViT-like images;
  long32k   one prompt of 32768 tokens, causal (this tool's own).

--heads-q / --heads-kv / --head-dim change the heads (a gpt-oss layer: 64 / 8 /
64).  --window W (causal batches) and --sinks run the backward through the
sliding window and the attention sinks (fa_attn_bwd_win_* / fa_attn_bwd_sink_*),
forward and backward with the same W and sinks.

One invocation = one batch and one dtype (run it under `timeout`), one JSON line.
Arms, alternated round by round after a warm-up (prefill_bench.py's loop):

  fwd    flash_attention_varlen with return_lse (what the backward recomputes from);
  bwd    the backward: three launches on out, lse and a fixed dout;
  sdpa   torch.nn.functional.scaled_dot_product_attention's backward alone
         (torch.autograd.grad on a retained graph, sequence by sequence, [1, H,
         n, D] with enable_gqa), whatever backend torch picks on the box;
  bwd_w0      with --window: the backward of the same batch (and sinks) without
              the window, on its own forward's out and lse;
  bwd_nosink  with --sinks: the backward at the same window without sinks;
  bwd2   `bwd` again: bwd_aa is the spread of the box.

Reported: the arms' times, bwd_over_fwd, bwd TFLOP/s by 10 Hq D sum n^2 (halved
under causal), sdpa_over_bwd (> 1: torch is slower), and the three kernels'
own times from torch.profiler (null where the profiler gives no kernel events;
with --sinks the dsinks reduction's too).  Beside the times stands the work the
mask leaves: tile_pairs, the (64-row query tile, 64-key tile) pairs that hold a
visible (row, key) pair, with tile_pairs_w0 and bwd_over_w0 / tiles_over_w0
under --window, so that a time ratio reads against a work ratio.  The SDPA arm
runs only without a window and sinks (torch's SDPA has neither).
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

KERNELS = ("delta", "dkdv", "dq", "dsinks")


def tile_pairs(n, causal, window):
    """The (64-row query tile, 64-key tile) pairs of self-attention sequences of
    n_b tokens that hold a visible (row, key) pair."""
    total = 0
    for nb in n:
        for r0 in range(0, nb, 64):
            r1 = min(nb, r0 + 64) - 1
            hi = r1 if causal else nb - 1
            lo = max(0, r0 - window + 1) if window > 0 else 0
            total += hi // 64 - lo // 64 + 1
    return total


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


def run(name, dt, rounds, iters, with_sdpa, hq=32, hkv=8, d=128, window=0, with_sinks=False):
    n, causal = ([32768], True) if name == "long32k" else selfattn_lengths(name)
    b = len(n)
    total = sum(n)
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    q, k, v, do = rnd(total, hq, d), rnd(total, hkv, d), rnd(total, hkv, d), rnd(total, hq, d)
    cu_host = [0] + [sum(n[:i + 1]) for i in range(b)]
    cu = torch.tensor(cu_host, dtype=torch.int32, device="cuda")
    sinks = (torch.rand(hq, generator=gen, device="cuda", dtype=torch.float32) * 4 - 2) if with_sinks else None
    grads = [torch.empty_like(t) for t in (q, k, v)]

    def backward_of(w, sk):
        """The backward at window w and sinks sk on that forward's own out and lse."""
        o, l = fa_mi355x.flash_attention_varlen(q, k, v, cu, causal=causal, return_lse=True, window=w, sinks=sk)
        ds = None if sk is None else torch.empty_like(sk)

        def f():
            return fa_mi355x.flash_attention_varlen_backward(do, q, k, v, o, l, cu, causal=causal, dq=grads[0],
                                                             dk=grads[1], dv=grads[2], window=w, sinks=sk, dsinks=ds)
        return f

    out = torch.empty_like(q)

    def fwd():
        return fa_mi355x.flash_attention_varlen(q, k, v, cu, causal=causal, out=out, return_lse=True,
                                                window=window, sinks=sinks)

    bwd = backward_of(window, sinks)
    arms, names = [fwd, bwd], ["fwd", "bwd"]
    rec = dict(batch_name=name, dtype=str(dt).split(".")[-1], causal=causal, batch=b, heads_q=hq, heads_kv=hkv,
               head_dim=d, total=total, max_n=max(n), rounds=rounds, iters=iters, window=window, sinks=with_sinks,
               tile_pairs=tile_pairs(n, causal, window))
    if window:
        arms.append(backward_of(0, sinks))
        names.append("bwd_w0")
        rec["tile_pairs_w0"] = tile_pairs(n, causal, 0)
    if with_sinks:
        arms.append(backward_of(window, None))
        names.append("bwd_nosink")
    if with_sdpa and not window and not with_sinks:
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
    # by the (row, key) pairs the mask leaves: n^2 / 2 under causal, less the triangle below a window
    pairs = sum((x * x * (0.5 if causal else 1.0)) - (0.5 * max(0, x - window) ** 2 if window else 0.0) for x in n)
    fl = 10.0 * hq * d * pairs
    rec["bwd_tflops"] = round(fl / (ts["bwd"][0] * 1e-3) / 1e12, 1)
    rec["fwd_tflops"] = round(0.4 * fl / (ts["fwd"][0] * 1e-3) / 1e12, 1)
    if window:
        rec["bwd_over_w0"] = round(ts["bwd"][0] / ts["bwd_w0"][0], 4)
        rec["tiles_over_w0"] = round(rec["tile_pairs"] / rec["tile_pairs_w0"], 4)
    if with_sinks:
        rec["bwd_over_nosink"] = round(ts["bwd"][0] / ts["bwd_nosink"][0], 4)
    rec["bwd_over_fwd"] = round(ts["bwd"][0] / ts["fwd"][0], 4)
    rec["bwd_aa"] = round(ts["bwd2"][0] / ts["bwd"][0], 4)
    if "sdpa" in ts:
        rec["sdpa_over_bwd"] = round(ts["sdpa"][0] / ts["bwd"][0], 4)
    kt = kernel_times(bwd, 5)
    rec["kernel_ms"] = {key: (round(val, 4) if isinstance(val, float) else val) for key, val in kt.items()}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", choices=SELFATTN + ("long32k",), required=True)
    ap.add_argument("--heads-q", type=int, default=32)
    ap.add_argument("--heads-kv", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=128, choices=(64, 128))
    ap.add_argument("--window", type=int, default=0, help="sliding window W (causal batches; 0: none)")
    ap.add_argument("--sinks", action="store_true", help="attention sinks, one per query head")
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
    rec = run(args.batch, dt, args.rounds, args.iters, not args.no_sdpa, args.heads_q, args.heads_kv,
              args.head_dim, args.window, args.sinks)
    rec["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
