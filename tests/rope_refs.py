"""References of the fused RoPE + cache append (fa_rope_append_*), on CPU
tensors: the table builder, the rotation by the contract's torch expression in
both pair styles, a float64 restatement of it, and the whole-tensor
expectations over a sentinel fill (the `_expect` of test_cache_append_gpu.py
restated with the `pos < rope_len` rule, and its twin for q_out)."""
import torch


def rope_tables(rope_len, r, base=10000.0):
    """cos, sin: float32 [rope_len, r / 2]; inv_freq = base^(-2i / r), angle = pos * inv_freq."""
    inv_freq = 1.0 / (base ** (torch.arange(0, r, 2, dtype=torch.float32) / r))
    ang = torch.outer(torch.arange(rope_len, dtype=torch.float32), inv_freq)
    return ang.cos().contiguous(), ang.sin().contiguous()


def _pairs(x, r, interleaved):
    if interleaved:
        return x[..., 0:r:2], x[..., 1:r:2]
    return x[..., :r // 2], x[..., r // 2:r]


def _join(x, ra, rb, r, interleaved):
    out = x.clone()
    if interleaved:
        out[..., 0:r:2], out[..., 1:r:2] = ra, rb
    else:
        out[..., :r // 2], out[..., r // 2:r] = ra, rb
    return out


def rotate(x, c, s, interleaved):
    """The contract: x [..., D] 16-bit, c / s float32 broadcastable to [..., R/2].
    Every product and sum is one fp32 torch operation, then one rounding."""
    r = 2 * c.shape[-1]
    a, b = (t.float() for t in _pairs(x, r, interleaved))
    return _join(x, (a * c - b * s).to(x.dtype), (b * c + a * s).to(x.dtype), r, interleaved)


def rotate_f64(x, c, s, interleaved):
    """The same in float64 (products exact, one rounding of the sum), rounded to x's dtype."""
    r = 2 * c.shape[-1]
    a, b = (t.double() for t in _pairs(x, r, interleaved))
    c, s = c.double(), s.double()
    return _join(x, (a * c - b * s).to(x.dtype), (b * c + a * s).to(x.dtype), r, interleaved)


def ordered(x):
    """16-bit patterns as integers in value order (+0 and -0 both 0): |difference| is the ulp distance."""
    i = x.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7fff), i)


def positions(lens, sn, new_lens=None):
    """pos [B, sn] (int64) and n [B]: pos[b, t] = lens[b] - n_b + t, the cache row the append writes."""
    n = torch.tensor([sn if new_lens is None else min(max(int(x), 0), sn) for x in
                      (lens if new_lens is None else new_lens)], dtype=torch.int64)
    pos = torch.tensor([int(x) for x in lens], dtype=torch.int64)[:, None] - n[:, None] + torch.arange(sn)[None]
    return pos, n


def rotate_tokens(x, cos, sin, lens, new_lens=None, interleaved=False):
    """x [B, H, Sn, D] rotated by each token's position.  Returns (rotated,
    valid [B, Sn]): valid = t < n_b and 0 <= pos < rope_len; rows that are not
    valid come back unrotated (no call writes them)."""
    pos, n = positions(lens, x.shape[2], new_lens)
    valid = (torch.arange(x.shape[2])[None] < n[:, None]) & (pos >= 0) & (pos < cos.shape[0])
    p = pos.clamp(0, cos.shape[0] - 1)
    rot = rotate(x, cos[p][:, None], sin[p][:, None], interleaved)
    return torch.where(valid[:, None, :, None], rot, x), valid


def expect_cache(cache, src, lens, new_lens=None, table=None, rope_len=None):
    """The append's contract with the rope_len rule, by torch indexing on the
    CPU.  cache: [B,Hkv,cap,D] or (table given) the pool [P,Hkv,page,D]; src:
    [B,Hkv,Sn,D] of cache's dtype, what the rows hold once written."""
    out = cache.clone()
    sn = src.shape[2]
    for b, ln in enumerate(lens):
        n = sn if new_lens is None else min(max(int(new_lens[b]), 0), sn)
        for t in range(n):
            r = int(ln) - n + t
            if rope_len is not None and r >= rope_len:
                continue
            if table is None:
                if 0 <= r < cache.shape[2]:
                    out[b, :, r] = src[b, :, t]
            elif 0 <= r < table.shape[1] * cache.shape[2]:
                pid = int(table[b, r // cache.shape[2]])
                if 0 <= pid < cache.shape[0]:
                    out[pid, :, r % cache.shape[2]] = src[b, :, t]
    return out


def expect_q(fill, q_rot, valid):
    """q_out over a sentinel fill: the valid rows of q_rot, `fill` elsewhere."""
    return torch.where(valid[:, None, :, None], q_rot, fill)
