#!/usr/bin/env python3
"""MLA cache-writer benchmark: fa_mi355x.flash_attention_mla_append[_paged] and
flash_attention_mla_indexer_append against the torch composition an MLA caller
writes without them, alternated in one process (tools/cache_append_bench.py's
protocol).

The composition of the latent append: RoPE of k_pe and of every head's q_pe as
torch kernels (the contract's fp32 expression, on cos / sin rows gathered per
token OUTSIDE the timed region), the rotated q_pe assigned into q_out[..., 512:]
(no cat of the 512 absorbed dims: that flatters the composition), the cat of
[c_kv | k_pe], for an FP8 cache the multiply by the reciprocal scale, the clamp
and .to(float8_e4m3fn), and an advanced-index assignment into the cache from
index tensors built once outside the timed region (which flatters it again).
Of the key writer: amax, the scale, the same quantise, and two assignments
(its bytes are compared but need not be equal: the contract divides by 448 in
IEEE fp32, which the eager GPU expression is not known to do; the exact check
is tests/test_mla_append_gpu.py's, against the CPU).

Per row: both sides are captured into HIP graphs of `iters` calls that rotate
through `copies` of the sources and destinations, and the graphs are replayed
alternately (ours, composition, ours again) between device events; medians
over `rounds`.  ours2 / ours is the row's own A/A spread.  bytes = what the
writer must move (sources read + rows and q_out slices written), over its time,
as a share of the 6.29 TB/s copy rate.  gate: the composition's time minus
ours exceeds the A/A difference.

    python3 tools/mla_append_bench.py [--out profiles/mla_append_bench.jsonl] [--quick]

Shapes: the prefill chunk (8 x 4096 tokens) and the decode step (B = 64), at 16
and 128 query heads, into the four latent cache forms (pages of 64), and the
key writer on both shapes, contiguous and paged.
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
DT = torch.float16


def shapes(quick):
    if quick:
        return [dict(name="quick B=2 Sn=256", b=2, sn=256, cap=512, copies=2, iters=4)]
    return [dict(name="prefill B=8 Sn=4096", b=8, sn=4096, cap=4096, copies=2, iters=4),
            dict(name="decode step B=64 Sn=1", b=64, sn=1, cap=8192, copies=2, iters=20)]


def placement(row, page_size, gen):
    """kv_lens, per-token positions, and per copy (block table, flat pool row of every token)."""
    b, sn, cap = row["b"], row["sn"], row["cap"]
    if sn == cap:
        lens = torch.full((b,), sn, dtype=torch.int32, device="cuda")
    else:
        lens = torch.randint(sn, cap + 1, (b,), generator=gen, device="cuda").to(torch.int32)
    pos = (lens.long()[:, None] - sn + torch.arange(sn, device="cuda")[None, :]).reshape(-1)
    bidx = torch.arange(b, device="cuda").repeat_interleave(sn)
    places = []
    for _ in range(row["copies"]):
        if page_size:
            mpp = cap // page_size
            tab = torch.randperm(b * mpp, generator=gen, device="cuda").view(b, mpp).to(torch.int32).contiguous()
            places.append((tab, tab.long()[bidx, pos // page_size] * page_size + pos % page_size))
        else:
            places.append((None, bidx * cap + pos))
    return lens, pos, places


def measure(legs_fn, copies, iters, rounds):
    """Warm up outside the captures, capture each side, replay (ours, composition, ours); sorted us per call."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in legs_fn:
            for i in range(copies):
                fn(i)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graphs = []
    for fn in legs_fn:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(iters):
                fn(i)
        g.replay()
        graphs.append(g)
    torch.cuda.synchronize()
    legs = (0, 1, 0)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)]
          for _ in legs]
    for r in range(rounds):
        for j, gi in enumerate(legs):
            ev[j][r][0].record()
            graphs[gi].replay()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    return [sorted(a.elapsed_time(c) * 1e3 / iters for a, c in e) for e in ev]


def report(head, ts, nbytes, same):
    med = [t[len(t) // 2] for t in ts]
    return dict(**head, bytes_moved=nbytes, bit_identical_to_composition=same,
                ours_us=round(med[0], 2), composition_us=round(med[1], 2), ours2_us=round(med[2], 2),
                ours_min_us=round(min(ts[0][0], ts[2][0]), 2), ours_max_us=round(max(ts[0][-1], ts[2][-1]), 2),
                composition_min_us=round(ts[1][0], 2), composition_max_us=round(ts[1][-1], 2),
                ours_aa=round(med[2] / med[0], 4), composition_over_ours=round(med[1] / med[0], 3),
                ours_gb_per_s=round(nbytes / med[0] / 1e3, 1),
                ours_share_of_copy_rate=round(nbytes / (med[0] * 1e-6) / COPY_RATE, 4),
                gate_faster_beyond_aa=bool(med[1] - med[0] > abs(med[2] - med[0])))


def rnd(gen, *s):
    return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(DT)


def run_latent(row, hq, page_size, kv8, rounds=9):
    b, sn, cap, copies, iters = row["b"], row["sn"], row["cap"], row["copies"], row["iters"]
    total = b * sn
    gen = torch.Generator(device="cuda").manual_seed(1)
    lens, pos, places = placement(row, page_size, gen)
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=torch.float32, device="cuda") / 64))
    ang = torch.outer(torch.arange(cap, dtype=torch.float32, device="cuda"), inv_freq)
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()  # [cap, 32]
    ctok, stok = cos[pos].contiguous(), sin[pos].contiguous()  # [T, 32]
    scale = torch.tensor([0.65], dtype=torch.float32, device="cuda")
    rcp = 1.0 / scale
    # kv_a's output [T, 576] (c_kv | k_pe) and q [T, Hq, 192] (q_nope | q_pe), read in place
    srcs = [(rnd(gen, total, 576), rnd(gen, total, hq, 192)) for _ in range(copies)]
    shape = (b * cap // page_size, page_size, 576) if page_size else (b, cap, 576)
    # [0]: ours, [1]: the composition's
    caches = [[torch.zeros(shape, dtype=torch.uint8 if kv8 else DT, device="cuda") for _ in range(copies)]
              for _ in range(2)]
    qouts = [[torch.zeros((total, hq, 576), dtype=DT, device="cuda") for _ in range(copies)] for _ in range(2)]

    def ours(i):
        c = i % copies
        (kv_a, q), (tab, _) = srcs[c], places[c]
        kw = dict(q_pe=q[..., 128:], q_out=qouts[0][c], cos=cos, sin=sin, ckv_scale=scale if kv8 else None)
        if page_size:
            fa_mi355x.flash_attention_mla_append_paged(kv_a[:, :512], kv_a[:, 512:], caches[0][c], tab, lens, **kw)
        else:
            fa_mi355x.flash_attention_mla_append(kv_a[:, :512], kv_a[:, 512:], caches[0][c], lens, **kw)

    def rope(x, c, s):
        a, bb = x[..., :32].float(), x[..., 32:].float()
        return torch.cat((a * c - bb * s, bb * c + a * s), -1).to(DT)

    def composition(i):
        c = i % copies
        (kv_a, q), (_, rows) = srcs[c], places[c]
        qouts[1][c][..., 512:] = rope(q[..., 128:], ctok[:, None], stok[:, None])
        latent = torch.cat((kv_a[:, :512], rope(kv_a[:, 512:], ctok, stok)), -1)
        if kv8:
            latent = torch.clamp(latent.float() * rcp, -448, 448).to(FP8).view(torch.uint8)
        caches[1][c].view(-1, 576)[rows] = latent

    ts = measure((ours, composition), copies, iters, rounds)
    same = all(torch.equal(a, c) for a, c in zip(*caches)) and all(torch.equal(a, c) for a, c in zip(*qouts))
    nbytes = total * (576 * 2 + 576 * (1 if kv8 else 2)) + total * hq * 64 * 2 * 2
    head = dict(name=row["name"], writer="latent", cache="kv8" if kv8 else "16-bit", page_size=page_size, batch=b,
                heads_q=hq, seqlen_new=sn, kv_capacity=cap, copies=copies, iters=iters, rounds=rounds)
    return report(head, ts, nbytes, same)


def run_indexer(row, page_size, rounds=9):
    b, sn, cap, copies, iters = row["b"], row["sn"], row["cap"], row["copies"], row["iters"]
    total = b * sn
    gen = torch.Generator(device="cuda").manual_seed(2)
    lens, _, places = placement(row, page_size, gen)
    srcs = [rnd(gen, total, 128) for _ in range(copies)]
    shape = (b * cap // page_size, page_size, 128) if page_size else (b, cap, 128)
    pools = [[torch.zeros(shape, dtype=torch.uint8, device="cuda") for _ in range(copies)] for _ in range(2)]
    scales = [[torch.zeros(b * cap, dtype=torch.float32, device="cuda") for _ in range(copies)] for _ in range(2)]

    def ours(i):
        c = i % copies
        fa_mi355x.flash_attention_mla_indexer_append(srcs[c], pools[0][c], lens, scales[0][c],
                                                     block_table=places[c][0])

    def composition(i):
        c = i % copies
        x, rows = srcs[c].float(), places[c][1]
        s = x.abs().amax(-1).clamp_min(1e-4) / 448.0
        pools[1][c].view(-1, 128)[rows] = torch.clamp(x * (1.0 / s)[:, None], -448, 448).to(FP8).view(torch.uint8)
        scales[1][c][rows] = s

    ts = measure((ours, composition), copies, iters, rounds)
    same = all(torch.equal(a, c) for a, c in zip(*pools)) and all(torch.equal(a, c) for a, c in zip(*scales))
    head = dict(name=row["name"], writer="indexer k8", cache="k8", page_size=page_size, batch=b, heads_q=0,
                seqlen_new=sn, kv_capacity=cap, copies=copies, iters=iters, rounds=rounds)
    return report(head, ts, total * (128 * 2 + 128 + 4), same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..",
                                                  "profiles", "mla_append_bench.jsonl"))
    ap.add_argument("--quick", action="store_true", help="one small shape (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mla_append_bench.py needs a GPU")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()

        for row in shapes(args.quick):
            for hq in (4,) if args.quick else (16, 128):
                for page_size in (0, 64):
                    for kv8 in (False, True):
                        emit(run_latent(row, hq, page_size, kv8))
            for page_size in (0, 64):
                emit(run_indexer(row, page_size))


if __name__ == "__main__":
    main()
