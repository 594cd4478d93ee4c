#!/usr/bin/env python3
"""MLA sparse indexer benchmark: fa_mi355x.flash_attention_mla_indexer (the
logits kernel and the selection) against what a caller does without it in
torch -- einsum -> relu -> weighted sum over the 64 heads -> torch.topk, which
materialises [N, 64, keys] fp32 (in token chunks of 512 for the prefill shape,
where it would be 34 GB) -- on the same inputs.  Five legs alternate round by
round in one process by tools/decode_bench.py's method: pair / torch / pair /
logits alone / selection alone, so every row carries its own A/A spread (aa,
the second pair leg over the first).

Shapes of a DeepSeek-V3.2 server, topk = 2048, 64 index heads of 128 dims,
fp16 and bf16 q, 16-bit and FP8 (E4M3 + one fp32 scale per row) keys: a prefill
chunk of 4096 tokens over the 32k keys of their sequence (causal ranges: token
i scores keys [0, 28672 + i]), and decode B = 64 over a contiguous [B, cap,
128] key cache at 32k and 128k keys.  Reported per row: the times, the counted
work (MFMA flops 2 * pairs * 64 * 128, VALU max/FMA element operations 2 *
pairs * 64, key bytes read once, logit bytes written, logit bytes the selection
reads in its five passes) and the rates they imply.

    python3 tools/mla_indexer_bench.py [--out profiles/mla_indexer_bench.jsonl] [--quick]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402
from decode_bench import time_pair  # noqa: E402

H, D, TOPK = 64, 128, 2048


def torch_indexer(q, k, w, scale, lens, per_seq, cap):
    """The torch composition: token n sees keys [0, lens[n]) of sequence n // per_seq; positions, not rows."""
    out = []
    for n0 in range(0, q.shape[0], 512):
        qs, ws, ls = q[n0:n0 + 512], w[n0:n0 + 512], lens[n0:n0 + 512]
        if per_seq == 1:  # decode: one key sequence per token
            kk = k.view(-1, cap, D)[n0:n0 + 512].to(q.dtype)
            s = torch.einsum("nhd,nld->nhl", qs, kk).float()
            sc = None if scale is None else scale.view(-1, cap)[n0:n0 + 512]
        else:
            s = torch.einsum("nhd,ld->nhl", qs, k.to(q.dtype)).float()
            sc = None if scale is None else scale[None, :]
        lg = (torch.relu(s) * ws[:, :, None]).sum(1)
        if sc is not None:
            lg = lg * sc
        lg = lg.masked_fill(torch.arange(cap, device=q.device)[None, :] >= ls[:, None], float("-inf"))
        out.append(lg.topk(TOPK, dim=-1).indices)
    return torch.cat(out)


def run(name, n, per_seq, cap, lens, dtype, k8, rounds=5):
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(n + cap)
    rows = cap * (n // per_seq)
    q = (torch.rand((n, H, D), generator=gen, device=dev) * 2 - 1).to(dtype)
    k = torch.rand((rows, D), generator=gen, device=dev) * 2 - 1
    k = k.to(torch.float8_e4m3fn) if k8 else k.to(dtype)
    scale = torch.rand(rows, generator=gen, device=dev) + 0.5 if k8 else None
    w = torch.rand((n, H), generator=gen, device=dev) * 2 - 1
    ks = (torch.arange(n, device=dev) // per_seq * cap).to(torch.int32)
    ke = ks + lens
    kw = dict(k_scale=scale) if k8 else {}
    logits = torch.empty((n, cap), dtype=torch.float32, device=dev)
    pair = lambda i: fa_mi355x.flash_attention_mla_indexer(q, k, w, ks, ke, topk=TOPK, max_len=cap, **kw)
    fns = [pair, lambda i: torch_indexer(q, k, w, scale, lens, per_seq, cap), pair,
           lambda i: fa_mi355x.flash_attention_mla_indexer_logits(q, k, w, ks, ke, out=logits, **kw),
           lambda i: fa_mi355x.flash_attention_mla_indexer_topk(logits, ks, ke, TOPK, num_rows=rows)]
    fns[3](0)
    # the share of torch's picks that are in the kernel's lists (torch rounds the scores to q's type first)
    member = torch.zeros((n, cap), dtype=torch.bool, device=dev)
    member.scatter_(1, (fns[0](0) - ks[:, None]).long(), True)
    agree = float(member.gather(1, fns[1](0)).float().mean())
    t_p, t_t, t_p2, t_l, t_s = time_pair(fns, 2 if n > 128 else 5, rounds)
    pairs = int(lens.sum())
    flops, valu = 2.0 * pairs * H * D, 2.0 * pairs * H
    kbytes, lbytes = rows * D * (1 if k8 else 2), pairs * 4
    return dict(name=name, dtype=str(dtype).split(".")[-1], keys="e4m3" if k8 else "16-bit", tokens=n, cap=cap,
                topk=TOPK, pairs=pairs, pair_us=round(t_p, 1), aa=round(t_p2 / t_p, 4), torch_us=round(t_t, 1),
                torch_over_pair=round(t_t / t_p, 2), logits_us=round(t_l, 1), select_us=round(t_s, 1),
                mfma_flops=flops, valu_elem_ops=valu, key_bytes=kbytes, logit_bytes=lbytes,
                select_read_bytes=5 * lbytes, logits_tflops=round(flops / (t_l * 1e-6) / 1e12, 1),
                logits_valu_gops=round(valu / (t_l * 1e-6) / 1e9, 1),
                logits_write_gbs=round(lbytes / (t_l * 1e-6) / 1e9, 1),
                select_read_gbs=round(5 * lbytes / (t_s * 1e-6) / 1e9, 1), list_overlap_with_torch=round(agree, 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/mla_indexer_bench.jsonl")
    ap.add_argument("--quick", action="store_true", help="fp16 only")
    args = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
    out = args.out or os.path.join(root, "profiles", "mla_indexer_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    dev = "cuda"
    cases = [("prefill N=4096 over 32k", 4096, 4096, 32768,
              (28673 + torch.arange(4096, device=dev)).to(torch.int32)),
             ("decode B=64 at 32k", 64, 1, 32768, torch.full((64,), 32768, dtype=torch.int32, device=dev)),
             ("decode B=64 at 128k", 64, 1, 131072, torch.full((64,), 131072, dtype=torch.int32, device=dev))]
    with open(out, "w") as f:
        for dtype in (torch.float16,) if args.quick else (torch.float16, torch.bfloat16):
            for k8 in (False, True):
                for name, n, per_seq, cap, lens in cases:
                    rec = run(name, n, per_seq, cap, lens, dtype, k8)
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
