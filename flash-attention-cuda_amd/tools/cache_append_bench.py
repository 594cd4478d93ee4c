#!/usr/bin/env python3
"""Cache-append benchmark: fa_mi355x.flash_attention_cache_append[_paged]
against the torch composition a user writes without it, alternated in one
process.

The composition: for a 16-bit cache an advanced-index assignment from device
index tensors (batch / row, or page / offset through the block table; the
index tensors are built once outside the timed region, which flatters the
composition: a serving loop rebuilds them every step); for an FP8 cache the
multiply by the reciprocal scale, the clamp and .to(float8_e4m3fn) before the
same assignment.

Per row: both sides are captured into HIP graphs of `iters` calls that rotate
through copies of the sources and of the caches (more than the 256-MiB
Infinity Cache in all on the prefill shape), and the graphs are replayed
alternately (append, composition, append again) between device events; medians
over `rounds`.  append2 / append is the row's own A/A spread.  bytes = what the
append must move (sources read + rows written), over the append's time, as a
share of the 6.29 TB/s copy rate.  gate: the composition's time minus the
append's exceeds the A/A difference.

    python3 tools/cache_append_bench.py [--out profiles/cache_append_bench.jsonl] [--quick]

Shapes: a bandwidth-bound prefill append (B=16, Hkv=8, Sn=4096, D=128) and the
decode step (B=64, Hkv=8, Sn=1), each into a contiguous cache and into pools of
page size 64 and 256, 16-bit and kv8.

--varlen: the packed entry flash_attention_cache_append_varlen[_paged] on
token-major [T, Hkv, D] sources with cu_seqlens against what a packed caller
does today -- scatter K and V into padded [B, Hkv, max n_b, D] copies, then the
padded append with new_lens -- by the same protocol, on the three ragged
batches of tools/prefill_bench.py --varlen (Hkv = 8, D = 128), into a
contiguous cache and a pool of page size 256, 16-bit and kv8; written to
profiles/cache_append_varlen_bench.jsonl.

--rope: the fused flash_attention_rope_append[_paged] (Hq = 32, NeoX style, R =
D) against torch RoPE of Q and K followed by the existing append, and the
existing append alone, by the same protocol (fused, composition, fused again,
append), on the two shapes above into a contiguous 16-bit cache and a kv8 pool
of page size 256.  bytes = Q in + Q out + K, V in + cache rows written; written
to profiles/cache_append_rope_bench.jsonl.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402

COPY_RATE = 6.29e12  # measured copy rate, bytes/s
FP8 = torch.float8_e4m3fn


def shapes(quick):
    rows = [dict(name="prefill B=16 Sn=4096", b=16, hkv=8, sn=4096, d=128, cap=4096, copies=3, iters=6),
            dict(name="decode step B=64 Sn=1", b=64, hkv=8, sn=1, d=128, cap=8192, copies=2, iters=20)]
    if quick:
        rows = [dict(name="quick B=2 Sn=256", b=2, hkv=2, sn=256, d=128, cap=512, copies=2, iters=4)]
    return rows


def run(row, page_size, kv8, rounds=9):
    dt = torch.float16
    b, hkv, sn, d, cap = row["b"], row["hkv"], row["sn"], row["d"], row["cap"]
    copies, iters = row["copies"], row["iters"]
    paged = page_size > 0
    gen = torch.Generator(device="cuda").manual_seed(1)
    cdt = torch.uint8 if kv8 else dt

    # lengths after the append: the prefill fills [0, Sn); the decode step lands anywhere
    if sn == cap:
        lens = torch.full((b,), sn, dtype=torch.int32, device="cuda")
    else:
        lens = torch.randint(sn, cap + 1, (b,), generator=gen, device="cuda").to(torch.int32)
    rows_ = (lens.long()[:, None] - sn + torch.arange(sn, device="cuda")[None, :]).reshape(-1)  # [B * Sn]
    bidx = torch.arange(b, device="cuda").repeat_interleave(sn)
    if paged:
        mpp = cap // page_size
        npages = b * mpp
        shape = (npages, hkv, page_size, d)
    else:
        shape = (b, hkv, cap, d)
    k_scale = torch.tensor([2.0 ** -(3 - (h & 1)) * 1.3 for h in range(hkv)], dtype=torch.float32, device="cuda")
    v_scale = torch.tensor([2.0 ** -(2 + (h & 1)) * 0.7 for h in range(hkv)], dtype=torch.float32, device="cuda")
    rk, rv = (1.0 / k_scale)[None, :, None, None], (1.0 / v_scale)[None, :, None, None]

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    srcs = [(rnd(b, hkv, sn, d), rnd(b, hkv, sn, d)) for _ in range(copies)]
    # [0]: the append's caches, [1]: the composition's; the same tables
    caches = [[(torch.zeros(shape, dtype=cdt, device="cuda"), torch.zeros(shape, dtype=cdt, device="cuda"))
               for _ in range(copies)] for _ in range(2)]
    tabs, idx = [], []
    for _ in range(copies):
        if paged:
            tab = torch.randperm(npages, generator=gen, device="cuda").view(b, mpp).to(torch.int32).contiguous()
            tabs.append(tab)
            idx.append((tab.long()[bidx, rows_ // page_size], rows_ % page_size))
        else:
            tabs.append(None)
            idx.append((bidx, rows_))
    scales = dict(k_scale=k_scale, v_scale=v_scale) if kv8 else {}

    def typed(c):
        return c.view(FP8) if kv8 else c

    def ours(i):
        c = i % copies
        (kn, vn), (kc, vc) = srcs[c], caches[0][c]
        if paged:
            fa_mi355x.flash_attention_cache_append_paged(kn, vn, typed(kc), typed(vc), tabs[c], lens, **scales)
        else:
            fa_mi355x.flash_attention_cache_append(kn, vn, typed(kc), typed(vc), lens, **scales)

    def composition(i):
        c = i % copies
        (kn, vn), (kc, vc), (i0, i1) = srcs[c], caches[1][c], idx[c]
        if kv8:
            kn = torch.clamp(kn.float() * rk, -448, 448).to(FP8).view(torch.uint8)
            vn = torch.clamp(vn.float() * rv, -448, 448).to(FP8).view(torch.uint8)
        kc[i0, :, i1] = kn.transpose(1, 2).reshape(b * sn, hkv, d)
        vc[i0, :, i1] = vn.transpose(1, 2).reshape(b * sn, hkv, d)

    legs_fn = (ours, composition)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in legs_fn:
            for i in range(copies):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(*caches))
    written = int((caches[0][0][0] != 0).sum())
    graphs = []
    for fn in legs_fn:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(iters):
                fn(i)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0)  # append, composition, append again (the A/A leg)
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
    elems = 2 * b * hkv * sn * d  # K and V
    nbytes = elems * 2 + elems * (1 if kv8 else 2)
    return dict(name=row["name"], cache="kv8" if kv8 else "16-bit", page_size=page_size, batch=b, heads_kv=hkv,
                seqlen_new=sn, head_dim=d, kv_capacity=cap, copies=copies, iters=iters, rounds=rounds,
                bytes_moved=nbytes, bit_identical_to_composition=same, nonzero_elements_written=written,
                append_us=round(med[0], 2), composition_us=round(med[1], 2), append2_us=round(med[2], 2),
                append_min_us=round(min(ts[0][0], ts[2][0]), 2), append_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                composition_min_us=round(ts[1][0], 2), composition_max_us=round(ts[1][-1], 2),
                append_aa=round(med[2] / med[0], 4), composition_over_append=round(med[1] / med[0], 3),
                append_gb_per_s=round(nbytes / med[0] / 1e3, 1),
                append_share_of_copy_rate=round(nbytes / (med[0] * 1e-6) / COPY_RATE, 4),
                gate_faster_beyond_aa=bool(med[1] - med[0] > abs(med[2] - med[0])))


def varlen_lengths(name):
    """(n_b, prefix_b): the batches of tools/prefill_bench.py --varlen."""
    if name == "uniform":
        return [4096] * 8, [0] * 8
    if name == "ragged":
        return [512 * (i + 1) for i in range(8)], [0] * 8
    return [4096] + [1 + (5 * i) % 16 for i in range(63)], [0] + [2048] * 63


def run_varlen(name, page_size, kv8, rounds=9, copies=2, iters=4):
    dt = torch.float16
    n, prefix = varlen_lengths(name)
    b, hkv, d = len(n), 8, 128
    total, smax = sum(n), max(n)
    kvl = [p + x for p, x in zip(prefix, n)]
    cap = -(-max(kvl) // 256) * 256
    paged = page_size > 0
    gen = torch.Generator(device="cuda").manual_seed(1)
    cdt = torch.uint8 if kv8 else dt
    cu = torch.tensor([0] + [sum(n[:i + 1]) for i in range(b)], dtype=torch.int32, device="cuda")
    lens = torch.tensor(kvl, dtype=torch.int32, device="cuda")
    new_lens = torch.tensor(n, dtype=torch.int32, device="cuda")
    idx_b = torch.repeat_interleave(torch.arange(b, device="cuda"), new_lens.long())
    idx_t = torch.arange(total, device="cuda") - cu[:-1].long()[idx_b]
    if paged:
        mpp = cap // page_size
        npages = b * mpp
        shape = (npages, hkv, page_size, d)
    else:
        shape = (b, hkv, cap, d)
    k_scale = torch.tensor([2.0 ** -(3 - (h & 1)) * 1.3 for h in range(hkv)], dtype=torch.float32, device="cuda")
    v_scale = torch.tensor([2.0 ** -(2 + (h & 1)) * 0.7 for h in range(hkv)], dtype=torch.float32, device="cuda")
    scales = dict(k_scale=k_scale, v_scale=v_scale) if kv8 else {}

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    srcs = [(rnd(total, hkv, d), rnd(total, hkv, d)) for _ in range(copies)]
    caches = [[(torch.zeros(shape, dtype=cdt, device="cuda"), torch.zeros(shape, dtype=cdt, device="cuda"))
               for _ in range(copies)] for _ in range(2)]
    tabs = [torch.randperm(npages, generator=gen, device="cuda").view(b, mpp).to(torch.int32).contiguous()
            if paged else None for _ in range(copies)]

    def typed(c):
        return c.view(FP8) if kv8 else c

    def ours(i):
        c = i % copies
        (kn, vn), (kc, vc) = srcs[c], caches[0][c]
        if paged:
            fa_mi355x.flash_attention_cache_append_varlen_paged(kn, vn, typed(kc), typed(vc), tabs[c], cu, lens,
                                                                **scales)
        else:
            fa_mi355x.flash_attention_cache_append_varlen(kn, vn, typed(kc), typed(vc), cu, lens, **scales)

    def scatter_padded(i):
        c = i % copies
        (kn, vn), (kc, vc) = srcs[c], caches[1][c]
        kpad = torch.empty((b, hkv, smax, d), dtype=dt, device="cuda")
        vpad = torch.empty((b, hkv, smax, d), dtype=dt, device="cuda")
        kpad[idx_b, :, idx_t] = kn
        vpad[idx_b, :, idx_t] = vn
        if paged:
            fa_mi355x.flash_attention_cache_append_paged(kpad, vpad, typed(kc), typed(vc), tabs[c], lens, new_lens,
                                                         **scales)
        else:
            fa_mi355x.flash_attention_cache_append(kpad, vpad, typed(kc), typed(vc), lens, new_lens, **scales)

    legs_fn = (ours, scatter_padded)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in legs_fn:
            for i in range(copies):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(*caches))
    graphs = []
    for fn in legs_fn:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(iters):
                fn(i)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0)  # packed, scatter + padded, packed again (the A/A leg)
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
    elems = 2 * total * hkv * d  # K and V
    nbytes = elems * 2 + elems * (1 if kv8 else 2)
    return dict(varlen=name, cache="kv8" if kv8 else "16-bit", page_size=page_size, batch=b, heads_kv=hkv,
                total_new=total, max_n=smax, padded_rows=b * smax, head_dim=d, kv_capacity=cap, copies=copies,
                iters=iters, rounds=rounds, bytes_moved=nbytes, bit_identical_to_scatter_padded=same,
                packed_us=round(med[0], 2), scatter_padded_us=round(med[1], 2), packed2_us=round(med[2], 2),
                packed_min_us=round(min(ts[0][0], ts[2][0]), 2), packed_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                scatter_padded_min_us=round(ts[1][0], 2), scatter_padded_max_us=round(ts[1][-1], 2),
                packed_aa=round(med[2] / med[0], 4), scatter_padded_over_packed=round(med[1] / med[0], 3),
                packed_gb_per_s=round(nbytes / med[0] / 1e3, 1),
                packed_share_of_copy_rate=round(nbytes / (med[0] * 1e-6) / COPY_RATE, 4))


def run_rope(row, page_size, kv8, hq=32, rounds=9):
    """--rope: flash_attention_rope_append[_paged] (NeoX style, R = D) against
    what a caller does today -- RoPE of Q and K as torch kernels (the contract's
    fp32 expression on cos / sin rows gathered per token OUTSIDE the timed
    region, which flatters the composition), then the existing append -- and
    the existing append alone.  Legs: fused, composition, fused again, append."""
    dt = torch.float16
    b, hkv, sn, d, cap = row["b"], row["hkv"], row["sn"], row["d"], row["cap"]
    copies, iters = row["copies"], row["iters"]
    paged = page_size > 0
    gen = torch.Generator(device="cuda").manual_seed(1)
    cdt = torch.uint8 if kv8 else dt
    if sn == cap:
        lens = torch.full((b,), sn, dtype=torch.int32, device="cuda")
    else:
        lens = torch.randint(sn, cap + 1, (b,), generator=gen, device="cuda").to(torch.int32)
    pos = lens.long()[:, None] - sn + torch.arange(sn, device="cuda")[None, :]  # [B, Sn]
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32, device="cuda") / d))
    ang = torch.outer(torch.arange(cap, dtype=torch.float32, device="cuda"), inv_freq)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()       # [cap, D/2]
    ctok, stok = cos[pos][:, None].contiguous(), sin[pos][:, None].contiguous()  # [B, 1, Sn, D/2]
    if paged:
        mpp = cap // page_size
        npages = b * mpp
        shape = (npages, hkv, page_size, d)
    else:
        shape = (b, hkv, cap, d)
    k_scale = torch.tensor([2.0 ** -(3 - (h & 1)) * 1.3 for h in range(hkv)], dtype=torch.float32, device="cuda")
    v_scale = torch.tensor([2.0 ** -(2 + (h & 1)) * 0.7 for h in range(hkv)], dtype=torch.float32, device="cuda")
    scales = dict(k_scale=k_scale, v_scale=v_scale) if kv8 else {}

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    srcs = [(rnd(b, hq, sn, d), rnd(b, hkv, sn, d), rnd(b, hkv, sn, d)) for _ in range(copies)]
    # [0]: the fused call's caches and q_out, [1]: the composition's, [2]: the plain append's
    caches = [[(torch.zeros(shape, dtype=cdt, device="cuda"), torch.zeros(shape, dtype=cdt, device="cuda"))
               for _ in range(copies)] for _ in range(3)]
    qouts = [[torch.zeros((b, hq, sn, d), dtype=dt, device="cuda") for _ in range(copies)] for _ in range(2)]
    tabs = [torch.randperm(npages, generator=gen, device="cuda").view(b, mpp).to(torch.int32).contiguous()
            if paged else None for _ in range(copies)]

    def typed(c):
        return c.view(FP8) if kv8 else c

    def plain(kn, vn, kc, vc, tab):
        if paged:
            fa_mi355x.flash_attention_cache_append_paged(kn, vn, typed(kc), typed(vc), tab, lens, **scales)
        else:
            fa_mi355x.flash_attention_cache_append(kn, vn, typed(kc), typed(vc), lens, **scales)

    def fused(i):
        c = i % copies
        (q, kn, vn), (kc, vc) = srcs[c], caches[0][c]
        if paged:
            fa_mi355x.flash_attention_rope_append_paged(q, kn, vn, typed(kc), typed(vc), tabs[c], lens, cos, sin,
                                                        q_out=qouts[0][c], **scales)
        else:
            fa_mi355x.flash_attention_rope_append(q, kn, vn, typed(kc), typed(vc), lens, cos, sin,
                                                  q_out=qouts[0][c], **scales)

    def rope_torch(x, out=None):
        a, bb = x[..., :d // 2].float(), x[..., d // 2:].float()
        y = torch.cat((a * ctok - bb * stok, bb * ctok + a * stok), -1)
        return y.to(dt) if out is None else out.copy_(y)

    def composition(i):
        c = i % copies
        (q, kn, vn), (kc, vc) = srcs[c], caches[1][c]
        rope_torch(q, qouts[1][c])
        plain(rope_torch(kn), vn, kc, vc, tabs[c])

    def append_alone(i):
        c = i % copies
        (_, kn, vn), (kc, vc) = srcs[c], caches[2][c]
        plain(kn, vn, kc, vc, tabs[c])

    legs_fn = (fused, composition, append_alone)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # first-launch set-up outside the captures
        for fn in legs_fn:
            for i in range(copies):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    same = all(torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) for a, c in zip(caches[0], caches[1])) \
        and all(torch.equal(a, c) for a, c in zip(*qouts))
    graphs = []
    for fn in legs_fn:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(iters):
                fn(i)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0, 2)  # fused, composition, fused again (the A/A leg), the plain append
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
    kv_elems = 2 * b * hkv * sn * d  # K and V
    q_elems = b * hq * sn * d
    nbytes = 2 * q_elems * 2 + kv_elems * 2 + kv_elems * (1 if kv8 else 2)  # Q in + Q out + K, V in + rows written
    plain_bytes = kv_elems * 2 + kv_elems * (1 if kv8 else 2)
    return dict(name=row["name"], rope="neox R=D", cache="kv8" if kv8 else "16-bit", page_size=page_size, batch=b,
                heads_q=hq, heads_kv=hkv, seqlen_new=sn, head_dim=d, kv_capacity=cap, copies=copies, iters=iters,
                rounds=rounds, bytes_moved=nbytes, bit_identical_to_composition=same,
                fused_us=round(med[0], 2), composition_us=round(med[1], 2), fused2_us=round(med[2], 2),
                append_alone_us=round(med[3], 2),
                fused_min_us=round(min(ts[0][0], ts[2][0]), 2), fused_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                composition_min_us=round(ts[1][0], 2), composition_max_us=round(ts[1][-1], 2),
                fused_aa=round(med[2] / med[0], 4), composition_over_fused=round(med[1] / med[0], 3),
                fused_gb_per_s=round(nbytes / med[0] / 1e3, 1),
                fused_share_of_copy_rate=round(nbytes / (med[0] * 1e-6) / COPY_RATE, 4),
                append_alone_share_of_copy_rate=round(plain_bytes / (med[3] * 1e-6) / COPY_RATE, 4),
                gate_faster_beyond_aa=bool(med[1] - med[0] > abs(med[2] - med[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..",
                                                  "profiles", "cache_append_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="one small shape (a rehearsal, not a measurement)")
    ap.add_argument("--varlen", action="store_true",
                    help="the packed entry against scatter + padded append (default --out: "
                         "profiles/cache_append_varlen_bench.jsonl)")
    ap.add_argument("--rope", action="store_true",
                    help="the fused RoPE + append against torch RoPE + the append (default --out: "
                         "profiles/cache_append_rope_bench.jsonl)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cache_append_bench.py needs a GPU")
    if args.rope:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(os.path.dirname(args.out), "cache_append_rope_bench.jsonl")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in shapes(args.quick):
                for page_size, kv8 in ((0, False), (256, True)):
                    rec = run_rope(row, page_size, kv8, hq=4 if args.quick else 32)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
                    torch.cuda.empty_cache()
        return
    if args.varlen and args.out == ap.get_default("out"):
        args.out = os.path.join(os.path.dirname(args.out), "cache_append_varlen_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.varlen:
        with open(args.out, "w") as f:
            for name in ("uniform", "ragged", "skewed"):
                for page_size in (0, 256):
                    for kv8 in (False, True):
                        rec = run_varlen(name, page_size, kv8)
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                        print(json.dumps(rec), flush=True)
                        torch.cuda.empty_cache()
        return
    with open(args.out, "w") as f:
        for row in shapes(args.quick):
            for page_size in (0, 64, 256):
                for kv8 in (False, True):
                    rec = run(row, page_size, kv8)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
