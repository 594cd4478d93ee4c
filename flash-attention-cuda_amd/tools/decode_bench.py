#!/usr/bin/env python3
"""Decode-attention benchmark: fa_mi355x.flash_attention_decode against PyTorch
SDPA on the same inputs, alternated in one process.

Per shape: us per call (device events around a batch of calls, warmed), the
K/V bytes the algorithm needs (2 * B * Hkv * sum(len) * D * 2, from shapes)
over that time, that as a share of the 6.29 TB/s copy rate, the plan's
num_splits, the SDPA time, and host_us: the Python + ctypes time to enqueue one
call (a row whose us is no more than host_us is bound by the host, not by the
kernel), and graph_us: the same calls replayed from one captured HIP graph, i.e.
without the host between them.  Rows with B <= 8 also time the forced
alternatives of the split plan (CUs filled 1x, 2x, 4x).  Caches smaller than
the 256-MiB Infinity Cache are rotated through enough copies (>= 512 MiB in
all) that every call streams from HBM.

    python3 tools/decode_bench.py [--out profiles/decode_bench.jsonl] [--quick]

--paged times fa_decode_paged_* against fa_decode_* instead (run_paged):
the same K/V data as a randomly permuted page pool plus block table, page
sizes 64 and 256, at three shapes (B=64 len=8192 bandwidth-bound, B=8 len=8192
and B=1 len=32768 latency-bound).  Both entries are captured into HIP graphs
(no host between calls) and the graphs replayed alternately in one process, a
second contiguous leg included so that every row carries its own A/A spread:
the figure of record is paged_over_contig beside contig_aa.

    python3 tools/decode_bench.py --paged [--out profiles/decode_paged_bench.jsonl]

--kv8 times the FP8-cache entries fa_decode_kv8_* against fa_decode_* on the
same logical shape (run_kv8): the 16-bit cache and its E4M3 quantisation (one
scale per K/V head), both captured into HIP graphs and replayed alternately
16-bit / kv8 / 16-bit in one process, so every row carries its own A/A spread;
the figure of record is kv8_over_kv16 beside kv16_aa, and kv8's own bytes per
second against the copy rate.  Rows marked `paged` add fa_decode_paged_kv8_* on
the same bytes as a randomly permuted pool, page sizes 64 and 256, in the same
rotation.

    python3 tools/decode_bench.py --kv8 [--out profiles/decode_kv8_bench.jsonl]

--window W times the sliding-window entries fa_decode_win_* against fa_decode_*
on the same cache (run_window): B=64 and B=1 at len 32768, contiguous and as a
page pool (page 256), captured into HIP graphs and replayed alternately plain /
windowed / plain / paged windowed, so every row carries its own A/A spread.
The figure of record is win_over_plain beside plain_aa and tile_ratio, the
share of 64-key tiles the windowed launch iterates, counted from the shape.

    python3 tools/decode_bench.py --window 4096 [--out profiles/decode_window_bench.jsonl]

--sinks (composable with --window) times the attention-sink entries
fa_decode_sink_* (sinks drawn from N(0, 2) per head) against the entries a call
without sinks takes at the same window -- fa_decode_* at 0, where the `_sink`
entry runs the windowed kernel at W = capacity, fa_decode_win_* otherwise -- on
the --window rows and in the same way (run_sinks): base / sinks / base / paged
sinks, sink_over_base beside base_aa.

    python3 tools/decode_bench.py --sinks [--window 4096] [--out profiles/decode_sinks_bench.jsonl]

--tree (composable with --window) times the tree-masked entries fa_decode_tree_*
(include/fa_mi355x_tree.h) under a seeded random tree against their `_sink`
twins under the chain rule at the same shape, window and sinks (run_tree): B =
64 at 4k and 32k keys and B = 1 at 32k (split), Sq 4, 8 and 16, fp16 and bf16,
over the contiguous 16-bit cache and over a paged FP8 pool (page 256), captured
into HIP graphs and replayed alternately twin / tree / twin for each cache
form, so every row carries its own A/A spread: tree_over_sink beside sink_aa,
tree_pkv8_over_sink_pkv8 beside sink_pkv8_aa.  The fp16 rows add what a caller
does without the entries: one `_sink` decode call per root-to-leaf path of the
same tree on the same cache (paths_over_tree; the cache rows a real caller
would also rewrite per path are not counted), and SDPA with an explicit mask
on the GQA-expanded 16-bit cache (sdpa_over_tree; gathering and dequantising a
paged FP8 pool first is not counted either).

    python3 tools/decode_bench.py --tree [--window 4096] [--out profiles/decode_tree_bench.jsonl]
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402

COPY_RATE = 6.29e12  # measured copy rate, bytes/s
MAX_SPLITS = 64
try:  # does this torch's SDPA take grouped K/V heads itself?
    F.scaled_dot_product_attention(torch.zeros(1, 2, 1, 8), torch.zeros(1, 1, 2, 8),
                                   torch.zeros(1, 1, 2, 8), enable_gqa=True)
    HAS_GQA = True
except TypeError:
    HAS_GQA = False


def shapes(quick):
    rows = []
    for b in (1, 8, 64):
        for n in (2048, 8192, 32768):
            rows.append(dict(name=f"base B={b} len={n}", b=b, hq=32, hkv=8, sq=1, d=128, lens=[n] * b))
    rows.append(dict(name="long B=1 len=131072", b=1, hq=32, hkv=8, sq=1, d=128, lens=[131072]))
    rows.append(dict(name="speculative Sq=4", b=8, hq=32, hkv=8, sq=4, d=128, lens=[8192] * 8))
    rows.append(dict(name="MHA Hq=Hkv=32", b=8, hq=32, hkv=32, sq=1, d=128, lens=[8192] * 8))
    rows.append(dict(name="head_dim 64", b=8, hq=32, hkv=8, sq=1, d=64, lens=[8192] * 8))
    rows.append(dict(name="bf16", b=8, hq=32, hkv=8, sq=1, d=128, lens=[8192] * 8, bf16=True))
    b = 16
    rag = [max(1, round(math.exp(math.log(32768) * i / (b - 1)))) for i in range(b)]
    rows.append(dict(name="ragged 1..32768", b=b, hq=32, hkv=8, sq=1, d=128, lens=rag))
    return rows[:2] + rows[-1:] if quick else rows


def fill_splits(units, cap, cus, fill):
    """csrc/fa_decode_host.hpp decode_plan with kDecodeFill = fill."""
    if units >= cus:
        return 1
    return max(1, min(-(-cus * fill // units), max(1, cap // 256), MAX_SPLITS))


def time_pair(fns, iters, rounds):
    """Median us per call of each fn; fns alternate round by round."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in fns]
    for fn in fns:
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    for r in range(rounds):
        for j, fn in enumerate(fns):
            ev[j][r][0].record()
            for i in range(iters):
                fn(r * iters + i)
            ev[j][r][1].record()
    torch.cuda.synchronize()
    out = []
    for j in range(len(fns)):
        ts = sorted(a.elapsed_time(b) * 1e3 / iters for a, b in ev[j])
        out.append(ts[len(ts) // 2])
    return out


def host_us(fn, iters):
    """Host time per call: the enqueue loop alone, from an idle device, no sync inside."""
    import time

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e6 / iters


def graph_us(q, ks, vs, tl, iters, rounds=7):
    """Median us per call with the host out of the way: `iters` calls of the C
    entry (the plan's split, a workspace of this function's own) captured into
    one HIP graph, replayed `rounds` times between device events."""
    lib = fa_mi355x.load_library()
    b, hq, sq, d = q.shape
    hkv, cap = ks[0].shape[1], ks[0].shape[2]
    need = lib.fa_decode_ws_bytes(b, hq, hkv, sq, cap, d, 0)
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    fn = lib.fa_decode_bf16 if q.dtype is torch.bfloat16 else lib.fa_decode_f16

    def enqueue(st):
        for i in range(iters):
            rc = fn(q.data_ptr(), ks[i % len(ks)].data_ptr(), vs[i % len(vs)].data_ptr(), out.data_ptr(),
                    None, b, hq, hkv, sq, cap, d, tl.data_ptr() if tl is not None else None, 1, 0,
                    ws.data_ptr() if need else None, need, st)
            assert rc == 0, rc

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        enqueue(side.cuda_stream)  # first-launch set-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enqueue(torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(rounds)]
    for e0, e1 in ev:
        e0.record()
        graph.replay()
        e1.record()
    torch.cuda.synchronize()
    ts = sorted(e0.elapsed_time(e1) * 1e3 / iters for e0, e1 in ev)
    return ts[len(ts) // 2]


def run(row, cus):
    dt = torch.bfloat16 if row.get("bf16") else torch.float16
    b, hq, hkv, sq, d = row["b"], row["hq"], row["hkv"], row["sq"], row["d"]
    lens = row["lens"]
    cap = max(lens)
    ragged = min(lens) != cap
    kv_bytes = 2 * hkv * sum(lens) * d * 2
    alloc = 2 * b * hkv * cap * d * 2
    copies = max(1, min(32, -(-(512 << 20) // alloc)))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    ks = [rnd(b, hkv, cap, d) for _ in range(copies)]
    vs = [rnd(b, hkv, cap, d) for _ in range(copies)]
    q = rnd(b, hq, sq, d)
    tl = torch.tensor(lens, dtype=torch.int32, device="cuda") if ragged else None
    g = hq // hkv
    mask = None
    if ragged or sq > 1:  # bottom-right causal and per-batch lengths as an SDPA mask
        key = torch.arange(cap, device="cuda")[None, None, :]
        lim = torch.tensor(lens, device="cuda")[:, None, None] - sq + 1 + \
            torch.arange(sq, device="cuda")[None, :, None]
        mask = (key < lim)[:, None]
    if not HAS_GQA and g > 1:
        kx = [k.repeat_interleave(g, 1) for k in ks]
        vx = [v.repeat_interleave(g, 1) for v in vs]

    def dec(ns):
        return lambda i: fa_mi355x.flash_attention_decode(q, ks[i % copies], vs[i % copies], tl,
                                                          causal=True, num_splits=ns)

    def sdpa(i):
        if HAS_GQA:
            return F.scaled_dot_product_attention(q, ks[i % copies], vs[i % copies], attn_mask=mask,
                                                  enable_gqa=g > 1)
        if g > 1:
            return F.scaled_dot_product_attention(q, kx[i % copies], vx[i % copies], attn_mask=mask)
        return F.scaled_dot_product_attention(q, ks[i % copies], vs[i % copies], attn_mask=mask)

    # correctness of what is timed (SDPA is the comparison of record here)
    err = float((dec(0)(0).float() - sdpa(0).float()).abs().max())
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, cap, d)
    iters = 20 if kv_bytes < (1 << 30) else 5
    t_dec, t_sdpa = time_pair([dec(0), sdpa], iters, 7)
    rec = dict(name=row["name"], batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, head_dim=d,
               dtype=str(dt).split(".")[-1], kv_len_max=cap, kv_len_sum=sum(lens), copies=copies,
               num_splits=plan, us=round(t_dec, 2), kv_bytes=kv_bytes,
               gb_per_s=round(kv_bytes / t_dec / 1e3, 1),
               share_of_copy_rate=round(kv_bytes / (t_dec * 1e-6) / COPY_RATE, 4),
               sdpa_us=round(t_sdpa, 2), sdpa_over_decode=round(t_sdpa / t_dec, 2),
               sdpa_gqa="enable_gqa" if HAS_GQA else "kv_expanded", max_abs_diff_vs_sdpa=err,
               host_us=round(host_us(dec(0), iters), 2),
               graph_us=round(graph_us(q, ks, vs, tl, iters), 2))
    rec["graph_gb_per_s"] = round(kv_bytes / rec["graph_us"] / 1e3, 1)
    rec["graph_share_of_copy_rate"] = round(kv_bytes / (rec["graph_us"] * 1e-6) / COPY_RATE, 4)
    if b <= 8:
        rows_ = g * sq
        rw = 16 if rows_ <= 16 else (32 if rows_ <= 32 else 64)
        units = b * hkv * -(-rows_ // rw)
        alts = sorted({fill_splits(units, cap, cus, f) for f in (1, 2, 4)})
        names = {f"fill_{f}x": fill_splits(units, cap, cus, f) for f in (1, 2, 4)}
        ts = time_pair([dec(ns) for ns in alts], iters, 7)
        by_ns = dict(zip(alts, ts))
        rec["plan_alternatives"] = {k: dict(num_splits=ns, us=round(by_ns[ns], 2)) for k, ns in names.items()}
    return rec


def paged_shapes():
    return [dict(name=f"paged B={b} len={n}", b=b, hq=32, hkv=8, sq=1, d=128, n=n)
            for b, n in ((64, 8192), (8, 8192), (1, 32768))]


def run_paged(row, page_size, cus, placement="random", rounds=9):
    """Paged against contiguous decode on the same data: us per call from
    alternately replayed HIP graphs (contiguous, paged, contiguous again)."""
    lib = fa_mi355x.load_library()
    dt = torch.float16
    b, hq, hkv, sq, d, cap = row["b"], row["hq"], row["hkv"], row["sq"], row["d"], row["n"]
    mpp = cap // page_size
    npages = b * mpp
    kv_bytes = 2 * b * hkv * cap * d * 2
    copies = max(1, min(32, -(-(512 << 20) // kv_bytes)))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    def pool(x, perm):  # logical page (b, j) -> pool page perm[b * mpp + j]
        out = torch.empty((npages, hkv, page_size, d), dtype=dt, device="cuda")
        out[perm] = x.view(b, hkv, mpp, page_size, d).permute(0, 2, 1, 3, 4).reshape(
            npages, hkv, page_size, d)
        return out

    ks, vs, kps, vps, tabs = [], [], [], [], []
    for _ in range(copies):
        k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
        perm = torch.randperm(npages, generator=gen, device="cuda") if placement == "random" else \
            torch.arange(npages, device="cuda")
        ks.append(k), vs.append(v), kps.append(pool(k, perm)), vps.append(pool(v, perm))
        tabs.append(perm.view(b, mpp).to(torch.int32).contiguous())
    q = rnd(b, hq, sq, d)
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, cap, d)
    need = lib.fa_decode_ws_bytes(b, hq, hkv, sq, cap, d, 0)
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() if need else None
    outs = [torch.empty_like(q) for _ in range(2)]
    iters = 20 if kv_bytes < (1 << 30) else 5

    def contig(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[0].data_ptr(),
                                   None, b, hq, hkv, sq, cap, d, None, 1, 0, wsp, need, st)
            assert rc == 0, rc

    def paged(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_paged_f16(q.data_ptr(), kps[c].data_ptr(), vps[c].data_ptr(),
                                         outs[1].data_ptr(), None, b, hq, hkv, sq, d, npages, page_size,
                                         tabs[c].data_ptr(), mpp, None, 1, 0, wsp, need, st)
            assert rc == 0, rc

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        contig(side.cuda_stream)
        paged(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[0], outs[1]))  # both ran copy (iters - 1) % copies last
    graphs = []
    for fn in (contig, paged):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0)  # contiguous, paged, contiguous again (the A/A leg)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    ts = [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]
    med = [t[len(t) // 2] for t in ts]
    return dict(name=row["name"], page_size=page_size, placement=placement, batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq,
                head_dim=d, dtype="float16", kv_len=cap, num_pages=npages, copies=copies,
                num_splits=plan, kv_bytes=kv_bytes, rounds=rounds, iters=iters, bit_identical=same,
                contig_us=round(med[0], 2), paged_us=round(med[1], 2), contig2_us=round(med[2], 2),
                contig_min_us=round(min(ts[0][0], ts[2][0]), 2),
                contig_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                paged_min_us=round(ts[1][0], 2), paged_max_us=round(ts[1][-1], 2),
                paged_over_contig=round(med[1] / med[0], 4), contig_aa=round(med[2] / med[0], 4),
                contig_share_of_copy_rate=round(kv_bytes / (med[0] * 1e-6) / COPY_RATE, 4),
                paged_share_of_copy_rate=round(kv_bytes / (med[1] * 1e-6) / COPY_RATE, 4))


def kv8_shapes():
    base = dict(hq=32, hkv=8, sq=1, d=128)
    return [dict(base, name="B=64 len=8192", b=64, n=8192, paged=True),
            dict(base, name="B=64 len=32768", b=64, n=32768),
            dict(base, name="B=8 len=8192", b=8, n=8192, paged=True),
            dict(base, name="B=1 len=32768", b=1, n=32768, paged=True),
            dict(base, name="speculative: B=8 len=8192 Sq=4", b=8, n=8192, sq=4),
            dict(base, name="head_dim 64: B=8 len=8192", b=8, n=8192, d=64),
            dict(base, name="bf16: B=8 len=8192", b=8, n=8192, bf16=True)]


def run_kv8(row, cus, rounds=9):
    """The kv8 entry against the 16-bit entry on the same logical shape: us per
    call from alternately replayed HIP graphs (16-bit, kv8, 16-bit again, then
    the paged kv8 legs of rows that ask for them)."""
    lib = fa_mi355x.load_library()
    bf16 = bool(row.get("bf16"))
    dt = torch.bfloat16 if bf16 else torch.float16
    f8 = torch.float8_e4m3fn
    b, hq, hkv, sq, d, cap = row["b"], row["hq"], row["hkv"], row["sq"], row["d"], row["n"]
    kv16_bytes = 2 * b * hkv * cap * d * 2
    kv8_bytes = kv16_bytes // 2
    copies = max(1, min(32, -(-(512 << 20) // kv8_bytes)))  # the kv8 leg, too, streams >= 512 MiB
    page_sizes = (64, 256) if row.get("paged") else ()
    gen = torch.Generator(device="cuda").manual_seed(1)
    # values in [-1, 1) against scales of 2^-3 .. 2^-2: codes up to 8, every head its own scale
    k_scale = torch.tensor([2.0 ** -(3 - (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
    v_scale = torch.tensor([2.0 ** -(2 + (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    def quant(x, scale):
        return (x.float() / scale[None, :, None, None]).to(f8)

    def pool(x, perm, ps):  # logical page (b, j) -> pool page perm[b * mpp + j]
        mpp = cap // ps
        out = torch.empty((b * mpp, hkv, ps, d), dtype=torch.uint8, device="cuda")
        out[perm] = x.view(torch.uint8).view(b, hkv, mpp, ps, d).permute(0, 2, 1, 3, 4).reshape(
            b * mpp, hkv, ps, d)
        return out.view(f8)

    ks, vs, k8s, v8s = [], [], [], []
    pools = {ps: ([], [], []) for ps in page_sizes}
    for _ in range(copies):
        k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
        k8, v8 = quant(k, k_scale), quant(v, v_scale)
        ks.append(k), vs.append(v), k8s.append(k8), v8s.append(v8)
        for ps in page_sizes:
            npages = b * (cap // ps)
            perm = torch.randperm(npages, generator=gen, device="cuda")
            pools[ps][0].append(pool(k8, perm, ps))
            pools[ps][1].append(pool(v8, perm, ps))
            pools[ps][2].append(perm.view(b, cap // ps).to(torch.int32).contiguous())
    q = rnd(b, hq, sq, d)
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, cap, d)
    need = lib.fa_decode_ws_bytes(b, hq, hkv, sq, cap, d, 0)
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() if need else None
    outs = [torch.empty_like(q) for _ in range(2 + len(page_sizes))]
    iters = 20 if kv16_bytes < (1 << 30) else 5
    fn16 = lib.fa_decode_bf16 if bf16 else lib.fa_decode_f16
    fn8 = lib.fa_decode_kv8_bf16 if bf16 else lib.fa_decode_kv8_f16
    fnp8 = lib.fa_decode_paged_kv8_bf16 if bf16 else lib.fa_decode_paged_kv8_f16

    def kv16(st):
        for i in range(iters):
            c = i % copies
            rc = fn16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[0].data_ptr(), None,
                      b, hq, hkv, sq, cap, d, None, 1, 0, wsp, need, st)
            assert rc == 0, rc

    def kv8(st):
        for i in range(iters):
            c = i % copies
            rc = fn8(q.data_ptr(), k8s[c].data_ptr(), v8s[c].data_ptr(), outs[1].data_ptr(), None,
                     b, hq, hkv, sq, cap, d, None, 1, 0, wsp, need, st, k_scale.data_ptr(),
                     v_scale.data_ptr())
            assert rc == 0, rc

    def paged8(j, ps):
        kps, vps, tabs = pools[ps]

        def fn(st):
            for i in range(iters):
                c = i % copies
                rc = fnp8(q.data_ptr(), kps[c].data_ptr(), vps[c].data_ptr(), outs[2 + j].data_ptr(),
                          None, b, hq, hkv, sq, d, kps[c].shape[0], ps, tabs[c].data_ptr(), cap // ps,
                          None, 1, 0, wsp, need, st, k_scale.data_ptr(), v_scale.data_ptr())
                assert rc == 0, rc
        return fn

    fns = [kv16, kv8] + [paged8(j, ps) for j, ps in enumerate(page_sizes)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in fns:
            fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # every leg ran copy (iters - 1) % copies last: what the quantisation costs on this data,
    # and the paged legs' bits against the contiguous kv8 leg's
    quant_err = float((outs[1].float() - outs[0].float()).abs().max())
    same = all(bool(torch.equal(outs[1], outs[2 + j])) for j in range(len(page_sizes)))
    graphs = []
    for fn in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0) + tuple(2 + j for j in range(len(page_sizes)))
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    ts = [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]
    med = [t[len(t) // 2] for t in ts]
    rec = dict(name=row["name"], batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, head_dim=d,
               dtype=str(dt).split(".")[-1], kv_len=cap, copies=copies, num_splits=plan,
               kv16_bytes=kv16_bytes, kv8_bytes=kv8_bytes, rounds=rounds, iters=iters,
               kv16_us=round(med[0], 2), kv8_us=round(med[1], 2), kv16b_us=round(med[2], 2),
               kv16_min_us=round(min(ts[0][0], ts[2][0]), 2), kv16_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
               kv8_min_us=round(ts[1][0], 2), kv8_max_us=round(ts[1][-1], 2),
               kv8_over_kv16=round(med[1] / med[0], 4), kv16_aa=round(med[2] / med[0], 4),
               kv16_share_of_copy_rate=round(kv16_bytes / (med[0] * 1e-6) / COPY_RATE, 4),
               kv8_gb_per_s=round(kv8_bytes / med[1] / 1e3, 1),
               kv8_share_of_copy_rate=round(kv8_bytes / (med[1] * 1e-6) / COPY_RATE, 4),
               max_abs_diff_kv8_vs_kv16=quant_err)
    for j, ps in enumerate(page_sizes):
        t = med[3 + j]
        rec[f"paged{ps}_kv8_us"] = round(t, 2)
        rec[f"paged{ps}_kv8_over_kv8"] = round(t / med[1], 4)
        rec[f"paged{ps}_kv8_over_kv16"] = round(t / med[0], 4)
    if page_sizes:
        rec["paged_bit_identical"] = same
    return rec


def window_shapes():
    return [dict(name=f"window B={b} len=32768", b=b, hq=32, hkv=8, sq=1, d=128, n=32768) for b in (64, 1)]


def run_window(row, window, cus, page_size=256, rounds=9):
    """The windowed entry against the plain one on the same cache: us per call
    from alternately replayed HIP graphs (plain, windowed, plain again, paged
    windowed)."""
    lib = fa_mi355x.load_library()
    dt = torch.float16
    b, hq, hkv, sq, d, cap = row["b"], row["hq"], row["hkv"], row["sq"], row["d"], row["n"]
    mpp = cap // page_size
    npages = b * mpp
    kv_bytes = 2 * b * hkv * cap * d * 2
    copies = max(1, min(32, -(-(512 << 20) // kv_bytes)))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    ks, vs, kps, vps, tabs = [], [], [], [], []
    for _ in range(copies):
        k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
        perm = torch.randperm(npages, generator=gen, device="cuda")
        ks.append(k), vs.append(v)
        for x, dst in ((k, kps), (v, vps)):
            out = torch.empty((npages, hkv, page_size, d), dtype=dt, device="cuda")
            out[perm] = x.view(b, hkv, mpp, page_size, d).permute(0, 2, 1, 3, 4).reshape(
                npages, hkv, page_size, d)
            dst.append(out)
        tabs.append(perm.view(b, mpp).to(torch.int32).contiguous())
    q = rnd(b, hq, sq, d)
    wcap = fa_mi355x.decode_window_capacity(cap, sq, window)
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, cap, d)
    plan_w = fa_mi355x.decode_num_splits(b, hq, hkv, sq, wcap, d)
    need = max(lib.fa_decode_ws_bytes(b, hq, hkv, sq, cap, d, 0), lib.fa_decode_ws_bytes(b, hq, hkv, sq, wcap, d, 0))
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() if need else None
    outs = [torch.empty_like(q) for _ in range(3)]
    iters = 20 if kv_bytes < (1 << 30) else 5

    def plain(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[0].data_ptr(),
                                   None, b, hq, hkv, sq, cap, d, None, 1, 0, wsp, need, st)
            assert rc == 0, rc

    def win(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_win_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[1].data_ptr(),
                                       None, b, hq, hkv, sq, cap, d, None, 1, window, 0, wsp, need, st)
            assert rc == 0, rc

    def win_paged(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_win_paged_f16(q.data_ptr(), kps[c].data_ptr(), vps[c].data_ptr(),
                                             outs[2].data_ptr(), None, b, hq, hkv, sq, d, npages, page_size,
                                             tabs[c].data_ptr(), mpp, None, 1, window, 0, wsp, need, st)
            assert rc == 0, rc

    fns = (plain, win, win_paged)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in fns:
            fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[1], outs[2]))
    graphs = []
    for fn in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0, 2)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    ts = [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]
    med = [t[len(t) // 2] for t in ts]
    tiles = -(-cap // 64)
    tiles_w = tiles - max(0, cap - sq + 1 - window) // 64
    win_bytes = 2 * b * hkv * min(cap, window + sq - 1) * d * 2
    return dict(name=row["name"], window=window, batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq, head_dim=d,
                dtype="float16", kv_len=cap, page_size=page_size, copies=copies, num_splits=plan,
                num_splits_window=plan_w, rounds=rounds, iters=iters, paged_bit_identical=same,
                plain_us=round(med[0], 2), win_us=round(med[1], 2), plain2_us=round(med[2], 2),
                win_paged_us=round(med[3], 2), plain_min_us=round(min(ts[0][0], ts[2][0]), 2),
                plain_max_us=round(max(ts[0][-1], ts[2][-1]), 2), win_min_us=round(ts[1][0], 2),
                win_max_us=round(ts[1][-1], 2), win_over_plain=round(med[1] / med[0], 4),
                win_paged_over_plain=round(med[3] / med[0], 4), plain_aa=round(med[2] / med[0], 4),
                tiles=tiles, tiles_window=tiles_w, tile_ratio=round(tiles_w / tiles, 4),
                win_share_of_copy_rate=round(win_bytes / (med[1] * 1e-6) / COPY_RATE, 4),
                plain_share_of_copy_rate=round(kv_bytes / (med[0] * 1e-6) / COPY_RATE, 4))


def run_sinks(row, window, cus, page_size=256, rounds=9):
    """The `_sink` entry at `window` (0 included: the windowed kernel at W =
    capacity) against the entry a call without sinks takes at the same window
    (fa_decode_f16 at 0, fa_decode_win_f16 otherwise): us per call from
    alternately replayed HIP graphs (base, sinks, base again, paged sinks)."""
    lib = fa_mi355x.load_library()
    dt = torch.float16
    b, hq, hkv, sq, d, cap = row["b"], row["hq"], row["hkv"], row["sq"], row["d"], row["n"]
    mpp = cap // page_size
    npages = b * mpp
    kv_bytes = 2 * b * hkv * cap * d * 2
    copies = max(1, min(32, -(-(512 << 20) // kv_bytes)))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    ks, vs, kps, vps, tabs = [], [], [], [], []
    for _ in range(copies):
        k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
        perm = torch.randperm(npages, generator=gen, device="cuda")
        ks.append(k), vs.append(v)
        for x, dst in ((k, kps), (v, vps)):
            out = torch.empty((npages, hkv, page_size, d), dtype=dt, device="cuda")
            out[perm] = x.view(b, hkv, mpp, page_size, d).permute(0, 2, 1, 3, 4).reshape(
                npages, hkv, page_size, d)
            dst.append(out)
        tabs.append(perm.view(b, mpp).to(torch.int32).contiguous())
    q = rnd(b, hq, sq, d)
    sinks = torch.randn(hq, generator=gen, device="cuda", dtype=torch.float32) * 2.0 ** 0.5
    wcap = fa_mi355x.decode_window_capacity(cap, sq, window)
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, wcap, d)
    need = lib.fa_decode_ws_bytes(b, hq, hkv, sq, wcap, d, 0)
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() if need else None
    outs = [torch.empty_like(q) for _ in range(3)]
    iters = 20 if kv_bytes < (1 << 30) else 5

    def base(st):
        for i in range(iters):
            c = i % copies
            if window:
                rc = lib.fa_decode_win_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[0].data_ptr(),
                                           None, b, hq, hkv, sq, cap, d, None, 1, window, 0, wsp, need, st)
            else:
                rc = lib.fa_decode_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[0].data_ptr(),
                                       None, b, hq, hkv, sq, cap, d, None, 1, 0, wsp, need, st)
            assert rc == 0, rc

    def sink(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_sink_f16(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), outs[1].data_ptr(),
                                        None, b, hq, hkv, sq, cap, d, None, 1, window, sinks.data_ptr(), 0, wsp,
                                        need, st)
            assert rc == 0, rc

    def sink_paged(st):
        for i in range(iters):
            c = i % copies
            rc = lib.fa_decode_sink_paged_f16(q.data_ptr(), kps[c].data_ptr(), vps[c].data_ptr(),
                                              outs[2].data_ptr(), None, b, hq, hkv, sq, d, npages, page_size,
                                              tabs[c].data_ptr(), mpp, None, 1, window, sinks.data_ptr(), 0, wsp,
                                              need, st)
            assert rc == 0, rc

    fns = (base, sink, sink_paged)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in fns:
            fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = bool(torch.equal(outs[1], outs[2]))
    graphs = []
    for fn in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0, 2)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    ts = [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]
    med = [t[len(t) // 2] for t in ts]
    return dict(name=row["name"].replace("window", "sinks"), window=window, sinks=True, batch=b, heads_q=hq,
                heads_kv=hkv, seqlen_q=sq, head_dim=d, dtype="float16", kv_len=cap, page_size=page_size,
                copies=copies, num_splits=plan, rounds=rounds, iters=iters, paged_bit_identical=same,
                base_entry="win" if window else "plain", base_us=round(med[0], 2), sink_us=round(med[1], 2),
                base2_us=round(med[2], 2), sink_paged_us=round(med[3], 2),
                base_min_us=round(min(ts[0][0], ts[2][0]), 2), base_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                sink_min_us=round(ts[1][0], 2), sink_max_us=round(ts[1][-1], 2),
                sink_over_base=round(med[1] / med[0], 4), sink_paged_over_base=round(med[3] / med[0], 4),
                base_aa=round(med[2] / med[0], 4))


def tree_shapes():
    rows = []
    for bf16 in (False, True):
        for b, n in ((64, 4096), (64, 32768), (1, 32768)):
            for sq in (4, 8, 16):
                rows.append(dict(name=f"tree B={b} len={n} Sq={sq} {'bf16' if bf16 else 'fp16'}", b=b, hq=32,
                                 hkv=8, sq=sq, d=128, n=n, bf16=bf16))
    return rows


def run_tree(row, window, cus, page_size=256, rounds=9):
    """The `_tree` entries under a seeded random tree against the `_sink` twins
    under the chain rule, contiguous 16-bit and paged FP8: us per call from
    alternately replayed HIP graphs, and (fp16 rows) one twin call per
    root-to-leaf path and SDPA with an explicit mask."""
    import numpy as np

    lib = fa_mi355x.load_library()
    dt = torch.bfloat16 if row["bf16"] else torch.float16
    ty = "_bf16" if row["bf16"] else "_f16"
    b, hq, hkv, sq, d, cap = row["b"], row["hq"], row["hkv"], row["sq"], row["d"], row["n"]
    mpp = cap // page_size
    npages = b * mpp
    kv_bytes = 2 * b * hkv * cap * d * 2
    copies = max(1, min(32, -(-(512 << 20) // kv_bytes)))
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*shape):
        return (torch.rand(shape, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    ks, vs, kps, vps, tabs = [], [], [], [], []
    for _ in range(copies):
        k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
        perm = torch.randperm(npages, generator=gen, device="cuda")
        ks.append(k), vs.append(v)
        for x, dst in ((k, kps), (v, vps)):
            out = torch.empty((npages, hkv, page_size, d), dtype=torch.float8_e4m3fn, device="cuda")
            out[perm] = x.view(b, hkv, mpp, page_size, d).permute(0, 2, 1, 3, 4).reshape(
                npages, hkv, page_size, d).to(torch.float8_e4m3fn)
            dst.append(out)
        tabs.append(perm.view(b, mpp).to(torch.int32).contiguous())
    q = rnd(b, hq, sq, d)
    sinks = torch.randn(hq, generator=gen, device="cuda", dtype=torch.float32) * 2.0 ** 0.5
    # one seeded random tree, shared by the batch so that its paths are one call each
    rng = np.random.default_rng(sq)
    parents = [int(rng.integers(-1, t)) if t else -1 for t in range(sq)]
    mask = fa_mi355x.tree_mask_from_parents(torch.tensor([parents] * b, device="cuda"))
    leaves = [t for t in range(sq) if t not in parents]
    depth = [bin(int(m)).count("1") for m in mask[0].tolist()]
    paths = [depth[t] for t in leaves]  # tokens per root-to-leaf path
    wcap = fa_mi355x.decode_window_capacity(cap, sq, window)
    plan = fa_mi355x.decode_num_splits(b, hq, hkv, sq, wcap, d)
    need = max(lib.fa_decode_ws_bytes(b, hq, hkv, n, fa_mi355x.decode_window_capacity(cap, n, window), d, 0)
               for n in set(paths) | {sq})
    ws = torch.zeros(max(need, 1), dtype=torch.uint8, device="cuda")
    wsp = ws.data_ptr() if need else None
    outs = [torch.empty_like(q) for _ in range(5)]
    iters = 20 if kv_bytes < (1 << 30) else 5
    sp, mp = sinks.data_ptr(), mask.data_ptr()

    def contig(name, out, extra, nq=sq):
        fn = getattr(lib, name + ty)

        def enqueue(st):
            for i in range(iters):
                c = i % copies
                rc = fn(q.data_ptr(), ks[c].data_ptr(), vs[c].data_ptr(), out.data_ptr(), None, b, hq, hkv, nq,
                        cap, d, None, 1, window, sp, *extra, 0, wsp, need, st)
                assert rc == 0, rc
        return enqueue

    def paged8(name, out, extra):
        fn = getattr(lib, name + ty)

        def enqueue(st):
            for i in range(iters):
                c = i % copies
                rc = fn(q.data_ptr(), kps[c].data_ptr(), vps[c].data_ptr(), out.data_ptr(), None, b, hq, hkv, sq,
                        d, npages, page_size, tabs[c].data_ptr(), mpp, None, 1, window, sp, *extra, 0, wsp, need,
                        st, None, None)
                assert rc == 0, rc
        return enqueue

    def per_path(st):  # q's first rows stand for a path's tokens: the time, not the values
        for n in paths:
            contig("fa_decode_sink", outs[4], (), n)(st)

    fns = [contig("fa_decode_sink", outs[0], ()), contig("fa_decode_tree", outs[1], (mp,)),
           paged8("fa_decode_sink_paged_kv8", outs[2], ()), paged8("fa_decode_tree_paged_kv8", outs[3], (mp,))]
    legs = [0, 1, 0, 2, 3, 2]
    if not row["bf16"]:
        fns.append(per_path)
        legs.append(4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in fns:
            fn(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs = []
    for fn in fns:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(torch.cuda.current_stream().cuda_stream)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    ts = [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]
    med = [t[len(t) // 2] for t in ts]
    rec = dict(name=row["name"], tree=True, window=window, batch=b, heads_q=hq, heads_kv=hkv, seqlen_q=sq,
               head_dim=d, dtype="bfloat16" if row["bf16"] else "float16", kv_len=cap, page_size=page_size,
               copies=copies, num_splits=plan, rounds=rounds, iters=iters, parents=parents, paths=paths,
               sink_us=round(med[0], 2), tree_us=round(med[1], 2), sink2_us=round(med[2], 2),
               sink_min_us=round(min(ts[0][0], ts[2][0]), 2), sink_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
               tree_min_us=round(ts[1][0], 2), tree_max_us=round(ts[1][-1], 2),
               tree_over_sink=round(med[1] / med[0], 4), sink_aa=round(med[2] / med[0], 4),
               sink_pkv8_us=round(med[3], 2), tree_pkv8_us=round(med[4], 2), sink_pkv8_2_us=round(med[5], 2),
               tree_pkv8_over_sink_pkv8=round(med[4] / med[3], 4), sink_pkv8_aa=round(med[5] / med[3], 4))
    if not row["bf16"]:
        rec.update(paths_us=round(med[6], 2), paths_over_tree=round(med[6] / med[1], 4))
        # SDPA with the tree as an explicit mask on the GQA-expanded cache (window 0 only: the
        # mask below has no window)
        g = hq // hkv
        seen = torch.ones((b, 1, sq, cap), dtype=torch.bool, device="cuda")
        bits = (mask[:, :, None] >> torch.arange(sq, device="cuda")[None, None, :]) & 1
        seen[:, 0, :, cap - sq:] = bits.bool()
        if window:
            pos = cap - sq + torch.tensor(depth, device="cuda") - 1
            key = torch.arange(cap - sq, device="cuda")
            seen[:, 0, :, :cap - sq] = key[None, None, :] > (pos - window)[None, :, None]
        ke, ve = ks[0].repeat_interleave(g, 1), vs[0].repeat_interleave(g, 1)
        sd = time_pair([lambda i: F.scaled_dot_product_attention(q, ke, ve, attn_mask=seen)], 2, 3)[0]
        err = float((F.scaled_dot_product_attention(q, ke, ve, attn_mask=seen).float()
                     - fa_mi355x.flash_attention_decode(q, ks[0], vs[0], tree_mask=mask, window=window).float()
                     ).abs().max())
        rec.update(sdpa_us=round(sd, 2), sdpa_over_tree=round(sd / med[1], 4), sdpa_max_abs_diff=err)
        del ke, ve, seen
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default profiles/decode_bench.jsonl "
                    "(profiles/decode_paged_bench.jsonl with --paged, "
                    "profiles/decode_kv8_bench.jsonl with --kv8)")
    ap.add_argument("--quick", action="store_true", help="three rows only")
    ap.add_argument("--paged", action="store_true",
                    help="paged against contiguous decode, page sizes 64 and 256")
    ap.add_argument("--kv8", action="store_true",
                    help="the FP8-cache entries against the 16-bit ones on the same shapes")
    ap.add_argument("--window", type=int, default=0,
                    help="the sliding-window entries at this W against the plain ones")
    ap.add_argument("--sinks", action="store_true",
                    help="the attention-sink entries at --window (0 included) against the entries without "
                         "sinks at the same window")
    ap.add_argument("--tree", action="store_true",
                    help="the tree-masked entries under a random tree against the `_sink` twins under the chain "
                         "rule at --window (0 included), and against per-path calls and masked SDPA")
    ap.add_argument("--placement", choices=("random", "identity"), default="random",
                    help="--paged: pool pages under a random permutation (default) or in logical order")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles",
                                "decode_tree_bench.jsonl" if args.tree else
                                "decode_sinks_bench.jsonl" if args.sinks else
                                "decode_window_bench.jsonl" if args.window else
                                "decode_kv8_bench.jsonl" if args.kv8 else
                                "decode_paged_bench.jsonl" if args.paged else "decode_bench.jsonl")
    if not torch.cuda.is_available():
        sys.exit("decode_bench.py needs a GPU")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.tree:
        jobs = [(run_tree, (row, args.window, cus)) for row in tree_shapes()]
    elif args.sinks:
        jobs = [(run_sinks, (row, args.window, cus)) for row in window_shapes()]
    elif args.window:
        jobs = [(run_window, (row, args.window, cus)) for row in window_shapes()]
    elif args.kv8:
        jobs = [(run_kv8, (row, cus)) for row in kv8_shapes()]
    elif args.paged:
        jobs = [(run_paged, (row, ps, cus, args.placement)) for row in paged_shapes() for ps in (64, 256)]
    else:
        jobs = [(run, (row, cus)) for row in shapes(args.quick)]
    with open(args.out, "w") as f:
        for fn, a in jobs:
            rec = fn(*a)
            rec["cus"] = cus
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
