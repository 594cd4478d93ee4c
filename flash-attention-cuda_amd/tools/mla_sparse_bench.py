#!/usr/bin/env python3
"""MLA sparse attention benchmark: fa_mi355x.flash_attention_mla_sparse against
(a) what a caller does without it -- index_select the listed rows into a
scratch [N, topk, 576] cache, then flash_attention_mla_decode(causal=False) on
the copy -- and (b) flash_attention_mla_decode alone on a contiguous cache of
exactly topk keys per token, the same arithmetic with no gather: the floor.
Alternated in one process by tools/decode_bench.py's method, sparse / (a) /
sparse / (b) round by round, so every row carries its own A/A spread (aa, the
second sparse leg over the first) beside gather_decode_over_sparse and
sparse_over_contig.

Shapes a DeepSeek-V3.2 server runs over a pool of 64 x 32k latent rows (2.4
GB), topk = 2048, Hq = 128 and 16 (TP 8), fp16 and bf16: decode B = 64 with Sq
= 1 and 2 and B = 1 (token (b, t) lists distinct rows of element b's 32k), and
a prefill chunk of N = 4096 tokens of one sequence (its 32k rows).  Reported:
time per call, the bytes gathered (N * topk * 1152) over time as a share of
decode_bench's copy rate, and TFLOP/s by 2 * N * Hq * topk * (576 + 512).  The
index lists are rotated through enough sets (>= 512 MiB of rows in all) that
a call does not find its rows in the 256-MiB Infinity Cache because the call
before it fetched them; the prefill chunk's 38 MB of rows stay cache-resident
by the nature of the workload.

    python3 tools/mla_sparse_bench.py [--out profiles/mla_sparse_bench.jsonl] [--quick]

--kv8: fa_mi355x.flash_attention_mla_sparse_kv8 over the same pool as E4M3 bytes
(576 B per row), five legs alternated round by round: the kernel, the 16-bit
sparse kernel on the dequantised pool, the kernel again (aa), index_select of
the bytes into a scratch cache + flash_attention_mla_decode_kv8, and that
decode alone on pre-gathered rows (the floor).  fp16; decode B = 64, decode B =
1 and the prefill chunk; rows to profiles/mla_sparse_kv8_bench.jsonl.
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

DQK, DV, TOPK, SEQ, BATCH = 576, 512, 2048, 32768, 64


def draw_lists(n, per_seq, gen):
    """int32 [n, TOPK]: token i lists TOPK distinct rows of sequence i // per_seq."""
    keys = torch.rand((n, SEQ), generator=gen, device="cuda")
    rows = keys.topk(TOPK, dim=-1).indices  # distinct, in random order
    return (rows + (torch.arange(n, device="cuda") // per_seq * SEQ)[:, None]).to(torch.int32)


def run(name, n, per_seq, hq, dtype, pool, rounds=7):
    dev = "cuda"
    scale = 192 ** -0.5
    gathered = n * TOPK * DQK * 2
    copies = max(1, -(-(512 << 20) // gathered))
    gen = torch.Generator(device=dev).manual_seed(n * 131 + hq)
    q = (torch.rand((n, hq, DQK), generator=gen, device=dev) * 2 - 1).to(dtype)
    lists = [draw_lists(n, per_seq, gen) for _ in range(copies)]
    scratch = torch.empty((n, TOPK, DQK), dtype=dtype, device=dev)
    gather = lambda idx, out: torch.index_select(pool, 0, idx.view(-1), out=out.view(-1, DQK))
    contig = [scratch] if copies == 1 else [torch.empty_like(scratch) for _ in range(copies)]
    for idx, c in zip(lists, contig):
        gather(idx, c)
    q4 = q.view(n, hq, 1, DQK)
    kw = dict(softmax_scale=scale)
    sparse = lambda i: fa_mi355x.flash_attention_mla_sparse(q, pool, lists[i % copies], **kw)

    def gather_decode(i):
        gather(lists[i % copies], scratch)
        return fa_mi355x.flash_attention_mla_decode(q4, scratch, causal=False, **kw)

    fns = [sparse, gather_decode, sparse,
           lambda i: fa_mi355x.flash_attention_mla_decode(q4, contig[i % copies], causal=False, **kw)]
    out = fns[0](0)
    diff = float((out.float() - fns[1](0).view(n, hq, DV).float()).abs().max())
    iters = 20 if n <= 128 else 5
    t_s, t_a, t_s2, t_b = time_pair(fns, iters, rounds)
    return dict(name=name, dtype=str(dtype).split(".")[-1], tokens=n, heads_q=hq, topk=TOPK,
                regime="narrow" if hq <= 16 else "wide", num_splits=fa_mi355x.mla_decode_num_splits(n, hq, 1, TOPK),
                list_sets=copies, sparse_us=round(t_s, 2), aa=round(t_s2 / t_s, 4),
                gather_decode_us=round(t_a, 2), gather_decode_over_sparse=round(t_a / t_s, 3),
                contig_us=round(t_b, 2), sparse_over_contig=round(t_s / t_b, 3),
                share_of_copy_rate=round(gathered / (t_s * 1e-6) / COPY_RATE, 4),
                tflops=round(2.0 * n * hq * TOPK * (DQK + DV) / (t_s * 1e-6) / 1e12, 2),
                max_abs_diff_vs_gather_decode=diff, nonfinite=int((~torch.isfinite(out)).sum()))


def run_kv8(name, n, per_seq, hq, pool8, pool16, sc, rounds=7):
    dev, dtype = "cuda", pool16.dtype
    scale = 192 ** -0.5
    gathered = n * TOPK * DQK
    copies = max(1, -(-(512 << 20) // gathered))
    gen = torch.Generator(device=dev).manual_seed(n * 131 + hq)
    q = (torch.rand((n, hq, DQK), generator=gen, device=dev) * 2 - 1).to(dtype)
    lists = [draw_lists(n, per_seq, gen) for _ in range(copies)]
    scratch = torch.empty((n, TOPK, DQK), dtype=torch.uint8, device=dev)
    gather = lambda idx, out: torch.index_select(pool8, 0, idx.view(-1), out=out.view(-1, DQK))
    contig = [scratch] if copies == 1 else [torch.empty_like(scratch) for _ in range(copies)]
    for idx, c in zip(lists, contig):
        gather(idx, c)
    q4 = q.view(n, hq, 1, DQK)
    kw = dict(softmax_scale=scale, ckv_scale=sc)
    sparse8 = lambda i: fa_mi355x.flash_attention_mla_sparse_kv8(q, pool8, lists[i % copies], scale, sc)

    def gather_decode(i):
        gather(lists[i % copies], scratch)
        return fa_mi355x.flash_attention_mla_decode_kv8(q4, scratch, causal=False, **kw)

    fns = [sparse8, lambda i: fa_mi355x.flash_attention_mla_sparse(q, pool16, lists[i % copies], softmax_scale=scale),
           sparse8, gather_decode,
           lambda i: fa_mi355x.flash_attention_mla_decode_kv8(q4, contig[i % copies], causal=False, **kw)]
    out = fns[0](0)
    diff = float((out.float() - fns[3](0).view(n, hq, DV).float()).abs().max())
    diff16 = float((out.float() - fns[1](0).float()).abs().max())
    iters = 20 if n <= 128 else 5
    t_s, t_16, t_s2, t_a, t_b = time_pair(fns, iters, rounds)
    return dict(name=name, dtype=str(dtype).split(".")[-1], tokens=n, heads_q=hq, topk=TOPK,
                regime="narrow" if hq <= 16 else "wide", num_splits=fa_mi355x.mla_decode_num_splits(n, hq, 1, TOPK),
                list_sets=copies, sparse_kv8_us=round(t_s, 2), aa=round(t_s2 / t_s, 4),
                sparse_16bit_us=round(t_16, 2), kv8_over_16bit=round(t_s / t_16, 3),
                gather_decode_kv8_us=round(t_a, 2), gather_decode_over_sparse=round(t_a / t_s, 3),
                contig_kv8_us=round(t_b, 2), sparse_over_contig=round(t_s / t_b, 3),
                share_of_copy_rate=round(gathered / (t_s * 1e-6) / COPY_RATE, 4),
                tflops=round(2.0 * n * hq * TOPK * (DQK + DV) / (t_s * 1e-6) / 1e12, 2),
                max_abs_diff_vs_gather_decode=diff, max_abs_diff_vs_16bit=diff16,
                nonfinite=int((~torch.isfinite(out)).sum()))


def main_kv8(out):
    """The --kv8 rows: E4M3 codes of magnitude <= 1 under the scale 0.75, and their exact fp16 image."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    shape = (BATCH * SEQ, DQK)
    pool8 = (torch.randint(0, 0x39, shape, generator=gen, device="cuda", dtype=torch.uint8)
             | (torch.randint(0, 2, shape, generator=gen, device="cuda", dtype=torch.uint8) << 7))
    sc = torch.tensor([0.75], dtype=torch.float32, device="cuda")
    pool16 = torch.empty(shape, dtype=torch.float16, device="cuda")
    for i in range(0, shape[0], 1 << 18):  # in slabs: no fp32 image of the whole pool
        pool16[i:i + (1 << 18)] = (pool8[i:i + (1 << 18)].view(torch.float8_e4m3fn).float() * 0.75).half()
    with open(out, "w") as f:
        for name, n, per_seq in (("decode B=64 Sq=1", BATCH, 1), ("decode B=1 Sq=1", 1, 1),
                                 ("prefill chunk N=4096", 4096, 4096)):
            for hq in (128, 16):
                rec = run_kv8(name, n, per_seq, hq, pool8, pool16, sc)
                print(json.dumps(rec), flush=True)
                f.write(json.dumps(rec) + "\n")
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/mla_sparse_bench.jsonl")
    ap.add_argument("--quick", action="store_true", help="decode B = 64 Sq = 1 only, fp16")
    ap.add_argument("--kv8", action="store_true", help="the FP8 pool's kernel and its four comparison legs")
    args = ap.parse_args()
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
    out = args.out or os.path.join(root, "profiles", "mla_sparse_kv8_bench.jsonl" if args.kv8
                                   else "mla_sparse_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    if args.kv8:
        return main_kv8(out)
    cases = [("decode B=64 Sq=1", BATCH, 1), ("decode B=64 Sq=2", 2 * BATCH, 2), ("decode B=1 Sq=1", 1, 1),
             ("prefill chunk N=4096", 4096, 4096)]
    with open(out, "w") as f:
        for dtype in (torch.float16,) if args.quick else (torch.float16, torch.bfloat16):
            gen = torch.Generator(device="cuda").manual_seed(1)
            pool = (torch.rand((BATCH * SEQ, DQK), generator=gen, device="cuda") * 2 - 1).to(dtype)
            for name, n, per_seq in cases[:1] if args.quick else cases:
                for hq in (128, 16):
                    rec = run(name, n, per_seq, hq, dtype, pool)
                    print(json.dumps(rec), flush=True)
                    f.write(json.dumps(rec) + "\n")
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
