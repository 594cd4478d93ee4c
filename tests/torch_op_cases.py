"""One valid call of each of the 46 overloads of torch.ops.fa_mi355x.* (test
infrastructure shared by test_torch_op_table_cpu.py and _gpu.py): the tensors,
the positional arguments of every overload, and the fa_mi355x function each
packet wraps.  D=64, Hq=2, Hkv=1, one sequence, a cache (or one page) of 64
keys, packed T=20 with cu=[0,20], rope tables [32,16], window 3, sinks [2]."""
import torch

T, CAP, D, HQ, HKV = 20, 64, 64, 2, 1
F16, F32, I32, F8 = torch.float16, torch.float32, torch.int32, torch.float8_e4m3fn

# packet -> (the fa_mi355x function it wraps, what the op passes on top of its own arguments)
WRAPPED = {"fwd": ("flash_attention_fwd", {}), "attn_varlen": ("flash_attention_varlen", {}),
           "attn_bshd": ("flash_attention_bshd", {}),
           "attn_varlen_fwd": ("flash_attention_varlen", {"return_lse": True}),
           "attn_bshd_fwd": ("flash_attention_bshd", {"return_lse": True}),
           "attn_varlen_bwd": ("flash_attention_varlen_backward", {}),
           "attn_bshd_bwd": ("flash_attention_bshd_backward", {})}
for _p in ("decode", "prefill", "prefill_varlen", "cache_append", "cache_append_varlen", "rope_append",
           "rope_append_varlen"):
    WRAPPED[_p] = ("flash_attention_" + _p, {})
    WRAPPED[_p + "_paged"] = ("flash_attention_" + _p + "_paged", {})


def inputs(new, ints, sq_decode, sq_prefill):
    """The tensors by name.  new(shape, dtype) makes a floating tensor, ints(values) an
    int32 one; the padded q has sq_decode rows for decode and sq_prefill for the rest."""
    t = {"qd": new((1, HQ, sq_decode, D), F16), "qp": new((1, HQ, sq_prefill, D), F16),
         "qt": new((T, HQ, D), F16), "kt": new((T, HKV, D), F16), "vt": new((T, HKV, D), F16),
         "kn": new((1, HKV, sq_prefill, D), F16), "vn": new((1, HKV, sq_prefill, D), F16),
         "kc": new((1, HKV, CAP, D), F16), "vc": new((1, HKV, CAP, D), F16),
         "kc8": new((1, HKV, CAP, D), F8), "vc8": new((1, HKV, CAP, D), F8),
         "ks": new((HKV,), F32).abs() + 0.5, "vs": new((HKV,), F32).abs() + 0.5,
         "bt": ints([[0]]), "cu": ints([0, T]), "kv": ints([40]), "ql": ints([sq_prefill]),
         "kv_pad": ints([20 + sq_prefill]), "kv_pack": ints([30]),  # after the append; positions < 32
         "cos": new((32, 16), F32), "sin": new((32, 16), F32), "sinks": new((HQ,), F32),
         "dout_t": new((T, HQ, D), F16), "out_t": new((T, HQ, D), F16), "lse_t": new((HQ, T), F32)}
    for n in ("qt", "kt", "vt", "dout_t", "out_t"):  # the same tokens as one [B,S,H,D] batch
        t[n[:-1] + "b"] = t[n].view(1, *t[n].shape)
    t["lse_b"] = t["lse_t"].view(HQ, 1, T).permute(1, 0, 2)
    return t


def cases(t):
    """[(packet, overload, args)]: the 46 overloads in registration order per packet."""
    win, snk = (3,), (3, t["sinks"])
    dense, paged = (t["kc"], t["vc"]), (t["kc"], t["vc"], t["bt"])
    rows = [("fwd", "default", (t["qp"], t["qp"], t["qp"], True))]
    for kind, q, lens in (("decode", t["qd"], (t["kv"],)), ("prefill", t["qp"], (t["kv"], t["ql"])),
                          ("prefill_varlen", t["qt"], (t["cu"], t["kv"]))):
        for packet, cache in ((kind, dense), (kind + "_paged", paged)):
            base = (q, *cache, *lens, True)
            if packet == "decode_paged":  # the default schema has no scales; .kv8 adds them
                rows += [(packet, "default", base),
                         (packet, "kv8", (q, t["kc8"], t["vc8"], t["bt"], *lens, True, t["ks"], t["vs"]))]
            else:
                rows.append((packet, "default", base + (None, None)))
            rows += [(packet, "window", base + (None, None) + win), (packet, "sinks", base + (None, None) + snk)]
    for cache, sfx in ((dense, ""), (paged, "_paged")):
        rows += [("cache_append" + sfx, "default", (t["kn"], t["vn"], *cache, t["kv_pad"], t["ql"], None, None)),
                 ("cache_append_varlen" + sfx, "default",
                  (t["kt"], t["vt"], *cache, t["cu"], t["kv_pack"], None, None)),
                 ("rope_append" + sfx, "default", (t["qp"], t["kn"], t["vn"], *cache, t["kv_pad"], t["cos"],
                                                   t["sin"], t["ql"], False, None, None)),
                 ("rope_append_varlen" + sfx, "default", (t["qt"], t["kt"], t["vt"], *cache, t["cu"],
                                                          t["kv_pack"], t["cos"], t["sin"], True, None, None))]
    for name, x, mid in (("attn_varlen", "t", (t["cu"], None)), ("attn_bshd", "b", ())):
        fwd = (t["q" + x], t["k" + x], t["v" + x], *mid, True)
        bwd = (t["dout_" + x], *fwd[:3], t["out_" + x], t["lse_" + x], *mid, True)
        for packet, args in ((name, fwd), (name + "_fwd", fwd), (name + "_bwd", bwd)):
            rows += [(packet, "default", args), (packet, "window", args + win), (packet, "sinks", args + snk)]
    return rows
