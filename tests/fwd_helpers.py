"""What several forward GPU test files share.  The three input generators draw
on the GPU and differ in where they round, so each file keeps the one whose
stream it had; the two references differ from the ones left in
test_persistent_gpu.py and test_split_gpu.py in fp32 operation order."""
import math

import numpy as np
import torch


def fa():
    import fa_mi355x

    return fa_mi355x


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.float16).cuda()


def to_host_bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def rand_half(shape, seed, scale=1.0):
    """fp16 uniform on [-0.5 * scale, 0.5 * scale), drawn in fp16."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.empty(shape, dtype=torch.float16, device="cuda")
    t.uniform_(-0.5 * scale, 0.5 * scale, generator=g)
    return t


def rand_cast(shape, seed, scale=1.0, dtype=torch.float16):
    """fp32 uniform on [-0.5 * scale, 0.5 * scale), then cast."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.empty(shape, dtype=torch.float32, device="cuda")
    t.uniform_(-0.5 * scale, 0.5 * scale, generator=g)
    return t.to(dtype)


def rand_scaled_cast(shape, seed, dtype=torch.float16, scale=1.0):
    """fp32 uniform on [-0.5, 0.5), times scale, then cast."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.empty(shape, dtype=torch.float32, device="cuda").uniform_(-0.5, 0.5, generator=g)
    return (t * scale).to(dtype)


def ref_fp32(q, k, v, causal):
    """fp32 attention of the 16-bit inputs, all heads at once."""
    q, k, v = q.float(), k.float(), v.float()
    s = (q @ k.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
    if causal:
        n = q.shape[-2]
        s = s.masked_fill(~torch.ones(n, n, device=q.device, dtype=torch.bool).tril(), float("-inf"))
    return torch.softmax(s, -1) @ v


def ref_fp32_by_head(q, k, v, causal):
    """fp32 attention of the 16-bit inputs, head by head (bounded memory)"""
    b, h, s, d = q.shape
    out = torch.empty((b, h, s, d), dtype=torch.float32, device=q.device)
    mask = torch.ones((s, s), dtype=torch.bool, device=q.device).tril() if causal else None
    for bi in range(b):
        for hi in range(h):
            sc = (q[bi, hi].float() @ k[bi, hi].float().t()) / math.sqrt(d)
            if causal:
                sc = sc.masked_fill(~mask, float("-inf"))
            out[bi, hi] = torch.softmax(sc, dim=-1) @ v[bi, hi].float()
    return out


# tier boundaries of the dispatcher (fa_fwd.hip select_tier / launch_auto):
# config 1 and its ragged neighbours (W4P pairs), few-head long causal (W4P
# pairs vs the workspace split tier), two rounds of pairs (quads), W4
# persistent from two rounds of 256-row items, the S <= 256 loop, the KV-quad
# under-filled non-causal case, the tail-pool shape class (>= 64 rounds per
# XCD, a reduced copy), d64 twins
BOUNDARY = [
    (1, 32, 1024, 128, True, False), (1, 32, 1023, 128, True, False), (1, 32, 1025, 128, True, False),
    (1, 32, 1024, 128, False, False), (1, 8, 4096, 128, True, False), (1, 4, 8192, 128, True, False),
    (2, 32, 1024, 128, True, False), (1, 16, 4096, 128, True, False), (4, 32, 1024, 128, True, False),
    (1, 32, 256, 128, True, False), (1, 32, 257, 128, False, False), (1, 32, 512, 128, False, False),
    (1, 32, 512, 128, True, False), (3, 5, 77, 128, True, False), (1, 1, 1, 128, False, False),
    (1, 32, 1024, 64, True, False), (1, 8, 4096, 64, True, False), (2, 16, 2048, 64, False, False),
    (1, 32, 1024, 128, True, True), (1, 4, 8192, 128, True, True), (1, 32, 2048, 64, True, True),
    # round 6: the singles / mixed edges (<= 1 block per CU; 1-2 per CU)
    (1, 32, 513, 128, True, False), (1, 32, 576, 128, True, False), (1, 17, 1024, 128, True, False),
    (1, 65, 256, 128, True, False), (1, 16, 1024, 64, False, False), (1, 16, 1088, 64, False, False),
    (1, 32, 768, 64, True, True), (1, 4, 4096, 128, False, True),
]
