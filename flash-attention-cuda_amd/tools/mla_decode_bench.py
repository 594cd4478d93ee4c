#!/usr/bin/env python3
"""MLA decode benchmark: fa_mi355x.flash_attention_mla_decode[_paged] against
the torch composition a caller with a latent cache runs without it (16-bit
q @ c^T, fp32 softmax with a length mask, @ c[..., :512]), alternated in one
process by tools/decode_bench.py's method: kernel / composition / kernel /
paged kernel round by round, so every row carries its own A/A spread (aa, the
second kernel leg over the first) beside composition_over_kernel and
paged_over_contig.

Shapes: B = 64 and 1, 4k and 32k keys, fp16 and bf16, at (Hq, Sq) = (16, 1) --
the narrow regime, reported as the share of decode_bench's copy rate on
B * len * 1152 bytes -- and (128, 1), (128, 2) -- the wide regime, reported as
TFLOP/s by 2 * rows * len * (576 + 512).  Every row holds both figures.  Caches
smaller than the 256-MiB Infinity Cache are rotated through enough copies
(>= 512 MiB in all) that every call streams from HBM.  The paged leg reads the
same bytes as a randomly permuted pool of 64-key pages; gathering them for the
composition is not counted.

    python3 tools/mla_decode_bench.py [--out profiles/mla_decode_bench.jsonl] [--quick]

--kv8: the FP8 latent cache's legs over the same shapes (fp16), kv8 kernel /
16-bit kernel on the dequantised cache (the baseline) / kv8 kernel / dequantise
into a 16-bit cache, then the 16-bit kernel (what a caller without the kv8
entries does) / paged kv8 kernel; the copy-rate share is on B * len * 576
bytes.  Default output profiles/mla_decode_kv8_bench.jsonl.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402
from decode_bench import COPY_RATE, time_pair  # noqa: E402

DQK, DV, PAGE = 576, 512, 64


def composition(q, c, mask, scale):
    b, hq, sq, _ = q.shape
    s = torch.matmul(q.view(b, hq * sq, DQK), c.transpose(1, 2)).float() * scale
    p = torch.softmax(s.masked_fill(mask[:, None, :], float("-inf")), -1).to(q.dtype)
    return torch.matmul(p, c[..., :DV]).view(b, hq, sq, DV)


def run(b, n, hq, sq, dtype, rounds=7):
    dev = "cuda"
    scale = 192 ** -0.5
    copies = max(1, -(-(512 << 20) // (b * n * DQK * 2)))
    gen = torch.Generator(device=dev).manual_seed(b * 131 + n + hq + sq)
    draw = lambda *shape: (torch.rand(shape, generator=gen, device=dev) * 2 - 1).to(dtype)
    q = draw(b, hq, sq, DQK)
    cs = [draw(b, n, DQK) for _ in range(copies)]
    lens = torch.full((b,), n, dtype=torch.int32, device=dev)
    mask = torch.arange(n, device=dev)[None, :] >= lens[:, None]
    perm = torch.randperm(b * n // PAGE, generator=gen, device=dev)
    table = torch.empty_like(perm)
    table[perm] = torch.arange(perm.numel(), device=dev)  # logical page i lives in pool page table[i]
    pools = [c.view(-1, PAGE, DQK)[perm].contiguous() for c in cs]
    table = table.view(b, n // PAGE).to(torch.int32)
    kw = dict(softmax_scale=scale, causal=False)
    fns = [lambda i: fa_mi355x.flash_attention_mla_decode(q, cs[i % copies], lens, **kw),
           lambda i: composition(q, cs[i % copies], mask, scale),
           lambda i: fa_mi355x.flash_attention_mla_decode(q, cs[i % copies], lens, **kw),
           lambda i: fa_mi355x.flash_attention_mla_decode_paged(q, pools[i % copies], table, lens, **kw)]
    nonfinite = [int((~torch.isfinite(fns[j](0))).sum()) for j in (0, 1)]  # kernel, composition
    diff = float((fns[0](0).float() - fns[1](0).float()).abs().max())
    same = bool(torch.equal(fns[0](0), fns[3](0)))
    iters = 20 if b * n <= 64 * 4096 else 5
    t_k, t_c, t_k2, t_p = time_pair(fns, iters, rounds)
    rows = hq * sq
    return dict(name=f"B={b} len={n} Hq={hq} Sq={sq}", dtype=str(dtype).split(".")[-1], regime="narrow" if rows <= 16 else "wide",
                num_splits=fa_mi355x.mla_decode_num_splits(b, hq, sq, n), copies=copies,
                kernel_us=round(t_k, 2), aa=round(t_k2 / t_k, 4), composition_us=round(t_c, 2),
                composition_over_kernel=round(t_c / t_k, 3), paged_us=round(t_p, 2),
                paged_over_contig=round(t_p / t_k, 4),
                share_of_copy_rate=round(b * n * 2 * DQK / (t_k * 1e-6) / COPY_RATE, 4),
                tflops=round(2.0 * b * rows * n * (DQK + DV) / (t_k * 1e-6) / 1e12, 2),
                max_abs_diff_vs_composition=diff, nonfinite_kernel=nonfinite[0],
                nonfinite_composition=nonfinite[1], paged_equals_contig=same)


def run_kv8(b, n, hq, sq, dtype, rounds=7):
    dev = "cuda"
    scale, ckv = 192 ** -0.5, 0.37
    copies = max(1, -(-(512 << 20) // (b * n * DQK)))
    gen = torch.Generator(device=dev).manual_seed(b * 131 + n + hq + sq)
    q = (torch.rand((b, hq, sq, DQK), generator=gen, device=dev) * 2 - 1).to(dtype)
    c8s = [((torch.rand((b, n, DQK), generator=gen, device=dev) * 2 - 1) / ckv).to(torch.float8_e4m3fn)
           for _ in range(copies)]
    sc = torch.tensor([ckv], dtype=torch.float32, device=dev)
    deq = lambda c8: (c8.to(torch.float32) * sc).to(dtype)
    c16s = [deq(c8) for c8 in c8s[:max(1, copies // 2)]]  # 16-bit rows are twice the bytes
    lens = torch.full((b,), n, dtype=torch.int32, device=dev)
    perm = torch.randperm(b * n // PAGE, generator=gen, device=dev)
    table = torch.empty_like(perm)
    table[perm] = torch.arange(perm.numel(), device=dev)
    pools = [c.view(-1, PAGE, DQK)[perm].contiguous() for c in c8s]
    table = table.view(b, n // PAGE).to(torch.int32)
    kw = dict(softmax_scale=scale, causal=False)
    kv8 = lambda i: fa_mi355x.flash_attention_mla_decode_kv8(q, c8s[i % copies], lens, ckv_scale=sc, **kw)
    fns = [kv8,
           lambda i: fa_mi355x.flash_attention_mla_decode(q, c16s[i % len(c16s)], lens, **kw),
           kv8,
           lambda i: fa_mi355x.flash_attention_mla_decode(q, deq(c8s[i % copies]), lens, **kw),
           lambda i: fa_mi355x.flash_attention_mla_decode_paged_kv8(q, pools[i % copies], table, lens, ckv_scale=sc,
                                                                    **kw)]
    diff = float((fns[0](0).float() - fns[1](0).float()).abs().max())
    same = bool(torch.equal(fns[0](0), fns[4](0)))
    iters = 20 if b * n <= 64 * 4096 else 5
    t_k, t_16, t_k2, t_dq, t_p = time_pair(fns, iters, rounds)
    rows = hq * sq
    return dict(name=f"B={b} len={n} Hq={hq} Sq={sq}", dtype=str(dtype).split(".")[-1],
                regime="narrow" if rows <= 16 else "wide",
                num_splits=fa_mi355x.mla_decode_num_splits(b, hq, sq, n), copies=copies,
                kv8_us=round(t_k, 2), aa=round(t_k2 / t_k, 4), kernel16_us=round(t_16, 2),
                kv8_over_kernel16=round(t_k / t_16, 4), dequant_then_kernel16_us=round(t_dq, 2),
                dequant_over_kv8=round(t_dq / t_k, 3), paged_us=round(t_p, 2), paged_over_contig=round(t_p / t_k, 4),
                share_of_copy_rate=round(b * n * DQK / (t_k * 1e-6) / COPY_RATE, 4),
                tflops=round(2.0 * b * rows * n * (DQK + DV) / (t_k * 1e-6) / 1e12, 2),
                max_abs_diff_vs_kernel16=diff, paged_equals_contig=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/mla_decode_bench.jsonl")
    ap.add_argument("--quick", action="store_true", help="B = 64 at 4k keys, fp16 only")
    ap.add_argument("--kv8", action="store_true", help="the FP8 latent cache's legs (fp16)")
    args = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
    out = args.out or os.path.join(root, "profiles", "mla_decode_kv8_bench.jsonl" if args.kv8 else "mla_decode_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for dtype in (torch.float16,) if args.quick or args.kv8 else (torch.float16, torch.bfloat16):
            for b, n in ((64, 4096),) if args.quick else ((64, 4096), (64, 32768), (1, 4096), (1, 32768)):
                for hq, sq in ((16, 1), (128, 1), (128, 2)):
                    rec = (run_kv8 if args.kv8 else run)(b, n, hq, sq, dtype)
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
