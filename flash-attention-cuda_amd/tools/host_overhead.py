"""Host-side cost per call of each entry path, on a shape whose kernel is far
shorter than the call (B=1 H=1 S=128, D=128): what a short launch pays before
the GPU sees it; for the op layer also a cache op (decode, one token of two
heads over a cache of capacity 256) through its default overload and through
its `.window` overload, and for the direct binding one function per call helper
(decode plain and windowed, prefill padded and packed, the append plain and with
RoPE, packed attention and its backward) on shapes as short.  Prints one JSON
line per path (microseconds per call, wall clock over N back-to-back calls,
then one synchronize).  Public API only: the same file measures any commit.

usage: python tools/host_overhead.py [--calls 3000] [--commit NAME --run N]
(--commit, --run: copied into each line, for an A/B of two checkouts)"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import fa_mi355x as fa  # noqa: E402
import fa_mi355x.torch_op  # noqa: E402,F401

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=3000)
ap.add_argument("--seq", type=int, default=128)
ap.add_argument("--commit", default=None)
ap.add_argument("--run", type=int, default=None)
a = ap.parse_args()
tag = {key: val for key, val in (("commit", a.commit), ("run", a.run)) if val is not None}

q, k, v = (torch.randn(1, 1, a.seq, 128, dtype=torch.float16, device="cuda") for _ in range(3))
o = torch.empty_like(q)
# decode: one token of two heads over a full cache of capacity 256
qd = torch.randn(1, 2, 1, 128, dtype=torch.float16, device="cuda")
kc, vc = (torch.randn(1, 2, 256, 128, dtype=torch.float16, device="cuda") for _ in range(2))
kv_lens = torch.full((1,), 256, dtype=torch.int32, device="cuda")
# the direct binding over that cache: a 16-token chunk (padded and packed), one
# appended token (plain and with RoPE), and packed attention with its backward
qp = torch.randn(1, 2, 16, 128, dtype=torch.float16, device="cuda")
qv = qp.transpose(1, 2).reshape(16, 2, 128).contiguous()
cu16 = torch.tensor([0, 16], dtype=torch.int32, device="cuda")
kn, vn = (torch.randn(1, 2, 1, 128, dtype=torch.float16, device="cuda") for _ in range(2))
cos, sin = (torch.randn(256, 64, dtype=torch.float32, device="cuda") for _ in range(2))
qa, ka, va, da = (torch.randn(a.seq, 2, 128, dtype=torch.float16, device="cuda") for _ in range(4))
cua = torch.tensor([0, a.seq], dtype=torch.int32, device="cuda")
oa, lsea = fa.flash_attention_varlen(qa, ka, va, cua, causal=True, return_lse=True)
lib = fa.load_library()
raw = (ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(k.data_ptr()), ctypes.c_void_p(v.data_ptr()),
       ctypes.c_void_p(o.data_ptr()), 1, 1, a.seq, 128, 1,
       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

# the same op registered through torch.library.custom_op (the round-1
# registration), to price custom_op's own dispatch layers
@torch.library.custom_op("fa_mi355x_customop::fwd", mutates_args=())
def _customop(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False) -> torch.Tensor:
    return fa.flash_attention_fwd(q, k, v, causal)


paths = {
    "c_abi_ctypes_raw": lambda: lib.fa_fwd_f16(*raw),
    "flash_attention_fwd(out=)": lambda: fa.flash_attention_fwd(q, k, v, True, out=o),
    "flash_attention_fwd": lambda: fa.flash_attention_fwd(q, k, v, True),
    "torch.ops.fa_mi355x.fwd": lambda: torch.ops.fa_mi355x.fwd(q, k, v, True),
    "torch.ops.fa_mi355x_customop.fwd (custom_op twin)": lambda: torch.ops.fa_mi355x_customop.fwd(q, k, v, True),
    "sdpa": lambda: F.scaled_dot_product_attention(q, k, v, is_causal=True),
    # a cache op through its default overload and through a later one (resolved by the packet)
    "torch.ops.fa_mi355x.decode": lambda: torch.ops.fa_mi355x.decode(qd, kc, vc, kv_lens, True),
    "torch.ops.fa_mi355x.decode.window": lambda: torch.ops.fa_mi355x.decode(qd, kc, vc, kv_lens, True, window=128),
    # the direct binding, one path per call helper
    "flash_attention_decode": lambda: fa.flash_attention_decode(qd, kc, vc, kv_lens),
    "flash_attention_decode(window=128)": lambda: fa.flash_attention_decode(qd, kc, vc, kv_lens, window=128),
    "flash_attention_prefill": lambda: fa.flash_attention_prefill(qp, kc, vc, kv_lens),
    "flash_attention_prefill_varlen": lambda: fa.flash_attention_prefill_varlen(qv, kc, vc, cu16, kv_lens),
    "flash_attention_cache_append": lambda: fa.flash_attention_cache_append(kn, vn, kc, vc, kv_lens),
    "flash_attention_rope_append": lambda: fa.flash_attention_rope_append(qd, kn, vn, kc, vc, kv_lens, cos, sin),
    "flash_attention_varlen": lambda: fa.flash_attention_varlen(qa, ka, va, cua, causal=True),
    "flash_attention_varlen_backward": lambda: fa.flash_attention_varlen_backward(da, qa, ka, va, oa, lsea, cua,
                                                                                 causal=True),
}
for name, fn in paths.items():
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps({**tag, "path": name, "seq": a.seq, "host_us_per_call": round((t1 - t0) / a.calls * 1e6, 2),
                      "wall_us_per_call": round((t2 - t0) / a.calls * 1e6, 2)}), flush=True)
