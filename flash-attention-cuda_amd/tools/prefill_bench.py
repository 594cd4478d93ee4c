#!/usr/bin/env python3
"""Prefill-attention benchmark: fa_mi355x.flash_attention_prefill[_paged] over
the four cache forms against what a caller had before it, arms alternated in
one process (modelled on tools/decode_bench.py).

One invocation = one shape and one dtype (run it under `timeout`), one JSON
line per cache form.  Per form, interleaved round by round after a warm-up:

  prefill   the new entry on the cache as it is (kv_lens / q_lens on the device);
  (a) fwd   flash_attention_fwd at Hq = Hkv = heads_q and S = Skv on 16-bit
            tensors: the asm tiers' kernel-only yardstick, reported as a ratio of
            TFLOP/s -- NOT a bar (a plain-C++ 4-wave loop sits below W4);
  (b) expand_fwd   no-prefix shapes only: what a caller must do without the
            entry -- gather pages / dequantise / repeat_interleave K and V to
            Hq heads into a scratch copy, then flash_attention_fwd -- timed
            whole, with the scratch bytes it allocates;
  (c) sdpa  prefix shapes only: PyTorch SDPA (enable_gqa, explicit bottom-right
            mask) on the gathered, dequantised cache (the gather and
            dequantisation are NOT in its time: it is charged the kernel only).

TFLOP/s uses the reference's convention extended to the contract:
4 * Hq * D * sum_b sum_t vis(b, t).

    timeout 300 python3 tools/prefill_bench.py --shape headline --dtype fp16 \\
        [--forms contig,paged,contig_kv8,paged_kv8] [--out profiles/prefill_bench.jsonl]

--varlen NAME (instead of --shape): the packed (cu_seqlens, token-major Q) entry
flash_attention_prefill_varlen[_paged] on a ragged batch at D = 128, Hq = 32,
Hkv = 8, three arms on the same lengths and cache, alternated the same way:

  packed    the packed entry on Q [T, Hq, D] and cu_seqlens;
  padded    the padded entry alone on inputs already in ITS layout (Q
            [B, Hq, max n_b, D] with q_lens = n, the rest padding): the yardstick;
  whole     what a packed caller pays today: scatter Q into the padded layout,
            the padded entry, gather O back (the padded buffers come from
            torch's caching allocator inside the arm).

    timeout 300 python3 tools/prefill_bench.py --varlen skewed [--out profiles/prefill_varlen_bench.jsonl]

--window W (with --shape): the sliding-window entry at this W against the entry
without a window on the same inputs, alternated the same way, plain / windowed
/ plain, so every row carries its own A/A spread.  The figure of record is
win_over_plain beside plain_aa and tile_ratio, the share of (query block, key
tile) pairs the windowed launch iterates, counted from the shape.

    timeout 300 python3 tools/prefill_bench.py --shape s32k --window 4096 [--out profiles/prefill_window_bench.jsonl]

--sinks (with --shape, composable with --window): the attention-sink entry
(sinks drawn from N(0, 2) per head) against the entry a call without sinks takes
at the same --window (0: the plain entry, against which the `_sink` entry runs
the windowed kernel at W = capacity), base / sinks / base: sink_over_base beside
base_aa.

    timeout 300 python3 tools/prefill_bench.py --shape s32k --window 4096 --sinks [--out profiles/prefill_sinks_bench.jsonl]

--selfattn NAME (instead of --shape): flash_attention_varlen, attention over
token-major Q, K and V with no cache, at D = 128, Hq = 32, Hkv = 8 on `uniform`
(8 prompts of 4096 tokens, causal), `ragged` (the --varlen batch, causal) or
`vit` (a non-causal packed batch of ViT-like lengths), alternated the same way:

  new       the entry on dense [T, H, D] tensors;
  (a) append_prefill   what a caller did before it: cache_append_varlen into a
            scratch contiguous cache (from torch's caching allocator inside the
            arm), then prefill_varlen on it;
  (b) prefill   prefill_varlen alone on a cache filled beforehand: the same K/V
            bytes through contiguous rows;
  fused     the entry on Q, K and V as the head slices of one [T, Hq + 2 Hkv, D]
            buffer, read in place (the rows a runtime stride apart);
  new2      `new` again: new_aa is the spread of the box.

    timeout 300 python3 tools/prefill_bench.py --selfattn ragged [--out profiles/prefill_selfattn_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import fa_mi355x  # noqa: E402

FP8 = torch.float8_e4m3fn
PAGE = 256
SHAPES = {
    # name: (B, Hq, Hkv, Sq, prefix)
    "headline": (8, 32, 8, 4096, 0),
    "prefix": (8, 32, 8, 2048, 6144),
    "long": (1, 32, 8, 8192, 0),
    "short_chunk": (16, 32, 8, 512, 8192),
    # one long prompt (the --window rows)
    "s8k": (1, 32, 8, 8192, 0),
    "s16k": (1, 32, 8, 16384, 0),
    "s32k": (1, 32, 8, 32768, 0),
}
FORMS = ("contig", "paged", "contig_kv8", "paged_kv8")


def varlen_lengths(name):
    """(n_b, prefix_b) of the --varlen batches."""
    if name == "uniform":
        return [4096] * 8, [0] * 8
    if name == "ragged":
        return [512 * (i + 1) for i in range(8)], [0] * 8
    # one 4096-token prompt and 63 chunks of 1..16 tokens behind 2048-key prefixes
    return [4096] + [1 + (5 * i) % 16 for i in range(63)], [0] + [2048] * 63


VARLEN = ("uniform", "ragged", "skewed")


def flops(b, hq, d, sq, prefix):
    vis = sum(prefix + t + 1 for t in range(sq))
    return 4.0 * hq * d * b * vis


def time_arms(fns, iters, rounds, warm=2):
    """Median ms per call of each arm; the arms alternate round by round."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(rounds)] for _ in fns]
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    for r in range(rounds):
        for j, fn in enumerate(fns):
            ev[j][r][0].record()
            for _ in range(iters):
                fn()
            ev[j][r][1].record()
    torch.cuda.synchronize()
    out = []
    for j in range(len(fns)):
        ts = sorted(a.elapsed_time(b) / iters for a, b in ev[j])
        out.append((ts[len(ts) // 2], ts[0], ts[-1]))
    return out


def run(shape, dt, form, rounds, iters):
    b, hq, hkv, sq, prefix = SHAPES[shape]
    d, g = 128, hq // hkv
    skv = prefix + sq
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    q = rnd(b, hq, sq, d)
    k16, v16 = rnd(b, hkv, skv, d), rnd(b, hkv, skv, d)
    kv_lens = torch.full((b,), skv, dtype=torch.int32, device="cuda")
    q_lens = torch.full((b,), sq, dtype=torch.int32, device="cuda")
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    scales = {}
    k, v = k16, v16
    if kv8:
        ks = torch.tensor([2.0 ** -(3 - (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        vs = torch.tensor([2.0 ** -(2 + (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        k = (k16.float() / ks[None, :, None, None]).to(FP8)
        v = (v16.float() / vs[None, :, None, None]).to(FP8)
        scales = dict(k_scale=ks, v_scale=vs)
    table = None
    if paged:
        mpp = skv // PAGE
        perm = torch.randperm(b * mpp, generator=gen, device="cuda")

        def pool(x):
            out = torch.empty((b * mpp, hkv, PAGE, d), dtype=x.dtype, device="cuda")
            src = x.view(b, hkv, mpp, PAGE, d).permute(0, 2, 1, 3, 4).reshape(b * mpp, hkv, PAGE, d)
            out.view(torch.uint8)[perm] = src.contiguous().view(torch.uint8)
            return out

        k, v = pool(k), pool(v)
        table = perm.view(b, mpp).to(torch.int32).contiguous()
    out = torch.empty_like(q)

    def prefill():
        if paged:
            return fa_mi355x.flash_attention_prefill_paged(q, k, v, table, kv_lens, q_lens, out=out, **scales)
        return fa_mi355x.flash_attention_prefill(q, k, v, kv_lens, q_lens, out=out, **scales)

    def expanded():
        """The contiguous 16-bit Hq-head K and V a caller without the entry builds."""
        kk, vv = k, v
        if paged:
            kk = kk[table.long()].permute(0, 2, 1, 3, 4).reshape(b, hkv, skv, d)
            vv = vv[table.long()].permute(0, 2, 1, 3, 4).reshape(b, hkv, skv, d)
        if kv8:
            kk = (kk.float() * scales["k_scale"][None, :, None, None]).to(dt)
            vv = (vv.float() * scales["v_scale"][None, :, None, None]).to(dt)
        return kk, vv

    # (a): the forward kernel alone at Hq = Hkv and S = Skv
    fq, fk, fv = rnd(b, hq, skv, d), rnd(b, hq, skv, d), rnd(b, hq, skv, d)
    fo = torch.empty_like(fq)

    def fwd():
        return fa_mi355x.flash_attention_fwd(fq, fk, fv, causal=True, out=fo)

    arms, names = [prefill, fwd], ["prefill", "fwd"]
    rec = dict(shape=shape, form=form, dtype=str(dt).split(".")[-1], batch=b, heads_q=hq, heads_kv=hkv,
               seqlen_q=sq, prefix=prefix, head_dim=d, page_size=PAGE if paged else None, rounds=rounds,
               iters=iters)
    if prefix == 0:
        def expand_fwd():
            kk, vv = expanded()
            return fa_mi355x.flash_attention_fwd(q, kk.repeat_interleave(g, 1), vv.repeat_interleave(g, 1),
                                                 causal=True)

        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ref = expand_fwd()
        rec["expand_scratch_bytes"] = int(torch.cuda.max_memory_allocated() - base - ref.numel() * 2)
        arms.append(expand_fwd)
        names.append("expand_fwd")
    else:
        gk, gv = (x.contiguous() for x in expanded())
        key = torch.arange(skv, device="cuda")[None, :]
        mask = (key <= prefix + torch.arange(sq, device="cuda")[:, None])[None, None]

        def sdpa():
            return F.scaled_dot_product_attention(q, gk, gv, attn_mask=mask, enable_gqa=g > 1)

        ref = sdpa()
        arms.append(sdpa)
        names.append("sdpa")
    rec["max_abs_diff_vs_" + names[2]] = float((prefill().float() - ref.float()).abs().max())
    del ref
    ts = time_arms(arms, iters, rounds)
    fl = flops(b, hq, d, sq, prefix)
    fl_fwd = 4.0 * b * hq * d * skv * (skv + 1) / 2
    for name, (med, lo, hi) in zip(names, ts):
        rec[name + "_ms"] = round(med, 4)
        rec[name + "_min_ms"] = round(lo, 4)
        rec[name + "_max_ms"] = round(hi, 4)
    rec["prefill_tflops"] = round(fl / (ts[0][0] * 1e-3) / 1e12, 1)
    rec["fwd_tflops"] = round(fl_fwd / (ts[1][0] * 1e-3) / 1e12, 1)
    rec["prefill_over_fwd_rate"] = round(rec["prefill_tflops"] / rec["fwd_tflops"], 4)
    rec[names[2] + "_over_prefill"] = round(ts[2][0] / ts[0][0], 4)
    return rec


def window_tiles(sq, prefix, window, bm=128, bn=64):
    """(key tiles the plain launch iterates per head, those of the windowed one)."""
    plain = win = 0
    for q0 in range(0, sq, bm):
        nt = -(-min(prefix + sq, prefix + q0 + bm) // bn)
        plain += nt
        win += nt - max(0, prefix + q0 - window + 1) // bn
    return plain, win


def window_inputs(shape, dt, form):
    """(q, k, v, table, kv_lens, q_lens, scales) of the --window / --sinks rows."""
    b, hq, hkv, sq, prefix = SHAPES[shape]
    d = 128
    skv = prefix + sq
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    q = rnd(b, hq, sq, d)
    k, v = rnd(b, hkv, skv, d), rnd(b, hkv, skv, d)
    kv_lens = torch.full((b,), skv, dtype=torch.int32, device="cuda")
    q_lens = torch.full((b,), sq, dtype=torch.int32, device="cuda")
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    scales = {}
    if kv8:
        ks = torch.tensor([2.0 ** -(3 - (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        vs = torch.tensor([2.0 ** -(2 + (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        k = (k.float() / ks[None, :, None, None]).to(FP8)
        v = (v.float() / vs[None, :, None, None]).to(FP8)
        scales = dict(k_scale=ks, v_scale=vs)
    table = None
    if paged:
        mpp = skv // PAGE
        perm = torch.randperm(b * mpp, generator=gen, device="cuda")

        def pool(x):
            out = torch.empty((b * mpp, hkv, PAGE, d), dtype=x.dtype, device="cuda")
            src = x.view(b, hkv, mpp, PAGE, d).permute(0, 2, 1, 3, 4).reshape(b * mpp, hkv, PAGE, d)
            out.view(torch.uint8)[perm] = src.contiguous().view(torch.uint8)
            return out

        k, v = pool(k), pool(v)
        table = perm.view(b, mpp).to(torch.int32).contiguous()
    return q, k, v, table, kv_lens, q_lens, scales


def window_arm(inputs, w, o, sinks=None):
    q, k, v, table, kv_lens, q_lens, scales = inputs

    def fn():
        if table is not None:
            return fa_mi355x.flash_attention_prefill_paged(q, k, v, table, kv_lens, q_lens, out=o, window=w,
                                                           sinks=sinks, **scales)
        return fa_mi355x.flash_attention_prefill(q, k, v, kv_lens, q_lens, out=o, window=w, sinks=sinks,
                                                 **scales)
    return fn


def run_window(shape, dt, form, window, rounds, iters):
    b, hq, hkv, sq, prefix = SHAPES[shape]
    d, paged = 128, form.startswith("paged")
    inputs = window_inputs(shape, dt, form)
    q = inputs[0]
    outs = [torch.empty_like(q), torch.empty_like(q)]
    plain, win = window_arm(inputs, 0, outs[0]), window_arm(inputs, window, outs[1])
    ts = time_arms([plain, win, plain], iters, rounds)
    tp, tw = window_tiles(sq, prefix, window)
    rec = dict(shape=shape, form=form, window=window, dtype=str(dt).split(".")[-1], batch=b, heads_q=hq,
               heads_kv=hkv, seqlen_q=sq, prefix=prefix, head_dim=d, page_size=PAGE if paged else None,
               rounds=rounds, iters=iters)
    for name, (med, lo, hi) in zip(("plain", "win", "plain2"), ts):
        rec[name + "_ms"] = round(med, 4)
        rec[name + "_min_ms"] = round(lo, 4)
        rec[name + "_max_ms"] = round(hi, 4)
    rec["win_over_plain"] = round(ts[1][0] / ts[0][0], 4)
    rec["plain_aa"] = round(ts[2][0] / ts[0][0], 4)
    rec["tiles"], rec["tiles_window"], rec["tile_ratio"] = tp, tw, round(tw / tp, 4)
    # rows whose window covers every key they see must agree exactly
    rec["head_rows_bit_identical"] = bool(torch.equal(outs[0][:, :, :min(sq, window)],
                                                      outs[1][:, :, :min(sq, window)]))
    return rec


def run_sinks(shape, dt, form, window, rounds, iters):
    """The `_sink` entry at `window` (0 included: the Windowed kernel at W =
    capacity) against the entry a call without sinks takes at the same window
    (the plain one at 0), base / sinks / base."""
    b, hq, hkv, sq, prefix = SHAPES[shape]
    d, paged = 128, form.startswith("paged")
    inputs = window_inputs(shape, dt, form)
    q = inputs[0]
    outs = [torch.empty_like(q), torch.empty_like(q)]
    gen = torch.Generator(device="cuda").manual_seed(2)
    sinks = torch.randn(hq, generator=gen, device="cuda", dtype=torch.float32) * 2.0 ** 0.5
    base, snk = window_arm(inputs, window, outs[0]), window_arm(inputs, window, outs[1], sinks)
    ts = time_arms([base, snk, base], iters, rounds)
    rec = dict(shape=shape, form=form, window=window, sinks=True, dtype=str(dt).split(".")[-1], batch=b,
               heads_q=hq, heads_kv=hkv, seqlen_q=sq, prefix=prefix, head_dim=d,
               page_size=PAGE if paged else None, rounds=rounds, iters=iters,
               base_entry="win" if window else "plain")
    for name, (med, lo, hi) in zip(("base", "sink", "base2"), ts):
        rec[name + "_ms"] = round(med, 4)
        rec[name + "_min_ms"] = round(lo, 4)
        rec[name + "_max_ms"] = round(hi, 4)
    rec["sink_over_base"] = round(ts[1][0] / ts[0][0], 4)
    rec["base_aa"] = round(ts[2][0] / ts[0][0], 4)
    # a sink only ever shrinks a row: |O| <= |O without|, and somewhere strictly
    rec["shrinks"] = bool((outs[1].float().abs() <= outs[0].float().abs() + 1e-3).all())
    return rec


def run_varlen(name, dt, form, rounds, iters):
    n, prefix = varlen_lengths(name)
    b, hq, hkv, d = len(n), 32, 8, 128
    total, smax = sum(n), max(n)
    kvl = [p + x for p, x in zip(prefix, n)]
    cap = -(-max(kvl) // PAGE) * PAGE
    gen = torch.Generator(device="cuda").manual_seed(1)

    def rnd(*s):
        return (torch.rand(s, generator=gen, device="cuda", dtype=torch.float32) * 2 - 1).to(dt)

    qp = rnd(total, hq, d)
    k, v = rnd(b, hkv, cap, d), rnd(b, hkv, cap, d)
    cu = torch.tensor([0] + [sum(n[:i + 1]) for i in range(b)], dtype=torch.int32, device="cuda")
    kv_lens = torch.tensor(kvl, dtype=torch.int32, device="cuda")
    q_lens = torch.tensor(n, dtype=torch.int32, device="cuda")
    # packed row -> (sequence, token)
    idx_b = torch.repeat_interleave(torch.arange(b, device="cuda"), q_lens.long())
    idx_t = torch.arange(total, device="cuda") - cu[:-1].long()[idx_b]
    kv8, paged = form.endswith("kv8"), form.startswith("paged")
    scales = {}
    if kv8:
        ks = torch.tensor([2.0 ** -(3 - (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        vs = torch.tensor([2.0 ** -(2 + (h & 1)) for h in range(hkv)], dtype=torch.float32, device="cuda")
        k = (k.float() / ks[None, :, None, None]).to(FP8)
        v = (v.float() / vs[None, :, None, None]).to(FP8)
        scales = dict(k_scale=ks, v_scale=vs)
    table = None
    if paged:
        mpp = cap // PAGE
        perm = torch.randperm(b * mpp, generator=gen, device="cuda")

        def pool(x):
            out = torch.empty((b * mpp, hkv, PAGE, d), dtype=x.dtype, device="cuda")
            src = x.view(b, hkv, mpp, PAGE, d).permute(0, 2, 1, 3, 4).reshape(b * mpp, hkv, PAGE, d)
            out.view(torch.uint8)[perm] = src.contiguous().view(torch.uint8)
            return out

        k, v = pool(k), pool(v)
        table = perm.view(b, mpp).to(torch.int32).contiguous()
    qpad = torch.zeros((b, hq, smax, d), dtype=dt, device="cuda")
    qpad[idx_b, :, idx_t] = qp
    op, opad = torch.empty_like(qp), torch.empty_like(qpad)

    def padded_entry(q, out):
        if paged:
            return fa_mi355x.flash_attention_prefill_paged(q, k, v, table, kv_lens, q_lens, out=out, **scales)
        return fa_mi355x.flash_attention_prefill(q, k, v, kv_lens, q_lens, out=out, **scales)

    def packed():
        if paged:
            return fa_mi355x.flash_attention_prefill_varlen_paged(qp, k, v, table, cu, kv_lens, out=op, **scales)
        return fa_mi355x.flash_attention_prefill_varlen(qp, k, v, cu, kv_lens, out=op, **scales)

    def padded():
        return padded_entry(qpad, opad)

    def whole():
        q = torch.empty((b, hq, smax, d), dtype=dt, device="cuda")
        q[idx_b, :, idx_t] = qp
        return padded_entry(q, torch.empty_like(q))[idx_b, :, idx_t]

    same = bool(torch.equal(packed(), whole()))
    ts = time_arms([packed, padded, whole], iters, rounds)
    fl = 4.0 * hq * d * sum(p * x + x * (x + 1) // 2 for p, x in zip(prefix, n))
    rec = dict(varlen=name, form=form, dtype=str(dt).split(".")[-1], batch=b, heads_q=hq, heads_kv=hkv,
               head_dim=d, total_q=total, max_n=smax, padded_rows=b * smax, kv_capacity=cap,
               page_size=PAGE if paged else None, rounds=rounds, iters=iters,
               packed_grid=hq * (total // 128 + b), padded_grid=b * hq * (-(-smax // 128)),
               packed_equals_whole_path=same)
    for arm, (med, lo, hi) in zip(("packed", "padded", "whole"), ts):
        rec[arm + "_ms"] = round(med, 4)
        rec[arm + "_min_ms"] = round(lo, 4)
        rec[arm + "_max_ms"] = round(hi, 4)
    rec["packed_tflops"] = round(fl / (ts[0][0] * 1e-3) / 1e12, 1)
    rec["padded_tflops"] = round(fl / (ts[1][0] * 1e-3) / 1e12, 1)
    rec["packed_over_padded"] = round(ts[0][0] / ts[1][0], 4)
    rec["whole_over_packed"] = round(ts[2][0] / ts[0][0], 4)
    return rec


SELFATTN = ("uniform", "ragged", "vit")


def selfattn_lengths(name):
    """(n_b, causal) of the --selfattn batches."""
    if name == "vit":
        # images of 14-pixel patches at mixed resolutions, each with a class token
        sides = [(16, 16), (24, 24), (32, 32), (27, 36), (37, 37), (18, 52), (64, 48), (32, 24)] * 4
        return [h * w + 1 for h, w in sides], False
    return varlen_lengths(name)[0], True


def run_selfattn(name, dt, rounds, iters):
    n, causal = selfattn_lengths(name)
    b, hq, hkv, d = len(n), 32, 8, 128
    total, cap = sum(n), -(-max(n) // 64) * 64
    gen = torch.Generator(device="cuda").manual_seed(1)
    fused = ((torch.rand((total, hq + 2 * hkv, d), generator=gen, device="cuda", dtype=torch.float32) * 2 - 1)
             .to(dt))
    fq, fk, fv = fused[:, :hq], fused[:, hq:hq + hkv], fused[:, hq + hkv:]
    q, k, v = fq.contiguous(), fk.contiguous(), fv.contiguous()
    cu = torch.tensor([0] + [sum(n[:i + 1]) for i in range(b)], dtype=torch.int32, device="cuda")
    kv_lens = torch.tensor(n, dtype=torch.int32, device="cuda")
    kc = torch.zeros((b, hkv, cap, d), dtype=dt, device="cuda")
    vc = torch.zeros_like(kc)
    fa_mi355x.flash_attention_cache_append_varlen(k, v, kc, vc, cu, kv_lens)
    outs = [torch.empty_like(q) for _ in range(4)]

    def new():
        return fa_mi355x.flash_attention_varlen(q, k, v, cu, causal=causal, out=outs[0])

    def append_prefill():
        k2 = torch.empty((b, hkv, cap, d), dtype=dt, device="cuda")
        v2 = torch.empty_like(k2)
        fa_mi355x.flash_attention_cache_append_varlen(k, v, k2, v2, cu, kv_lens)
        return fa_mi355x.flash_attention_prefill_varlen(q, k2, v2, cu, kv_lens, causal=causal, out=outs[1])

    def prefill():
        return fa_mi355x.flash_attention_prefill_varlen(q, kc, vc, cu, kv_lens, causal=causal, out=outs[2])

    def fused_views():
        return fa_mi355x.flash_attention_varlen(fq, fk, fv, cu, causal=causal, out=outs[3])

    same = bool(torch.equal(new(), append_prefill()) and torch.equal(outs[0], prefill())
                and torch.equal(outs[0], fused_views()))
    names = ("new", "append_prefill", "prefill", "fused", "new2")
    ts = time_arms([new, append_prefill, prefill, fused_views, new], iters, rounds)
    fl = 4.0 * hq * d * sum(x * (x + 1) // 2 if causal else x * x for x in n)
    rec = dict(selfattn=name, dtype=str(dt).split(".")[-1], causal=causal, batch=b, heads_q=hq, heads_kv=hkv,
               head_dim=d, total=total, max_n=max(n), scratch_cache_bytes=2 * b * hkv * cap * d * 2,
               rounds=rounds, iters=iters, bit_identical=same)
    for arm, (med, lo, hi) in zip(names, ts):
        rec[arm + "_ms"] = round(med, 4)
        rec[arm + "_min_ms"] = round(lo, 4)
        rec[arm + "_max_ms"] = round(hi, 4)
    rec["new_tflops"] = round(fl / (ts[0][0] * 1e-3) / 1e12, 1)
    rec["new_over_append_prefill"] = round(ts[0][0] / ts[1][0], 4)
    rec["new_over_prefill"] = round(ts[0][0] / ts[2][0], 4)
    rec["fused_over_prefill"] = round(ts[3][0] / ts[2][0], 4)
    rec["new_aa"] = round(ts[4][0] / ts[0][0], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--varlen", choices=VARLEN, help="a packed ragged batch instead of --shape")
    ap.add_argument("--selfattn", choices=SELFATTN,
                    help="attention over token-major Q, K, V with no cache instead of --shape")
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--window", type=int, default=0,
                    help="with --shape: the sliding-window entry at this W against the plain one")
    ap.add_argument("--sinks", action="store_true",
                    help="with --shape: the attention-sink entry at --window (0 included) against the entry "
                         "without sinks at the same window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=None, help="appended to; default profiles/prefill_bench.jsonl")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prefill_bench.py needs a GPU")
    if (args.shape is not None) + (args.varlen is not None) + (args.selfattn is not None) != 1:
        ap.error("one of --shape, --varlen and --selfattn is required")
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "profiles",
                                "prefill_varlen_bench.jsonl" if args.varlen else
                                "prefill_selfattn_bench.jsonl" if args.selfattn else
                                "prefill_sinks_bench.jsonl" if args.sinks else
                                "prefill_window_bench.jsonl" if args.window else "prefill_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    with open(args.out, "a") as f:
        if args.selfattn:
            rec = run_selfattn(args.selfattn, dt, args.rounds, args.iters)
            rec["cus"] = cus
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
            return
        for form in args.forms.split(","):
            assert form in FORMS, form
            if args.varlen:
                rec = run_varlen(args.varlen, dt, form, args.rounds, args.iters)
            elif args.sinks:
                rec = run_sinks(args.shape, dt, form, args.window, args.rounds, args.iters)
            elif args.window:
                rec = run_window(args.shape, dt, form, args.window, args.rounds, args.iters)
            else:
                rec = run(args.shape, dt, form, args.rounds, args.iters)
            rec["cus"] = cus
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
