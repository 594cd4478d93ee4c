"""The contract of the FP8 (E4M3) cache that cache append writes, twice: the
torch expression on the CPU (the reference the GPU tests compare with) and an
integer-only model of it (tests/test_cache_append_cpu.py pins one against the
other over every 16-bit pattern)."""
import numpy as np
import torch

FP8 = torch.float8_e4m3fn
NAN_PATTERNS = {torch.float16: 2046, torch.bfloat16: 254}


def torch_reference_bytes(x, scale):
    """E4M3 bytes (uint8 tensor) of the 16-bit CPU tensor `x` under the fp32
    scale `scale`: E4M3(clamp(float(x) * (1.0f / s), -448, 448)) by torch's CPU
    conversion.  The reciprocal is taken in double and rounded to fp32 by the
    multiplication, which equals the correctly rounded fp32 reciprocal (53 >=
    2 * 24 + 2 bits: the double rounding is innocuous)."""
    s = float(np.float32(scale))
    assert x.device.type == "cpu"
    return torch.clamp(x.float() * (1.0 / s), -448, 448).to(FP8).view(torch.uint8)


def _rne_scalar(m, sticky, nbits):
    """Python int m (with a sticky flag for bits below it) rounded to nearest
    even at nbits significant bits: (mantissa, bits shifted out)."""
    sh = max(m.bit_length() - nbits, 0)
    if sh == 0:
        return m, 0
    lo, half = m & ((1 << sh) - 1), 1 << (sh - 1)
    m >>= sh
    if lo > half or (lo == half and (sticky or (m & 1))):
        m += 1
    if m.bit_length() > nbits:
        m >>= 1
        sh += 1
    return m, sh


def _rne_shift(m, sh):
    """int64 array m >> sh (sh >= 1, elementwise), rounded to nearest even."""
    sh = np.minimum(sh, 62)
    q = m >> sh
    lo = m & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    return q + ((lo > half) | ((lo == half) & ((q & 1) == 1))).astype(np.int64)


def _bit_length(m):
    n = np.zeros(m.shape, dtype=np.int64)
    for k in range(48):
        n += (m >> k) > 0
    return n


def integer_reference_bytes(bits, dtype, scale):
    """The contract in integer arithmetic only.  bits: uint16 array of source
    patterns; returns (uint8 bytes, bool is_nan).  Steps: the correctly rounded
    fp32 reciprocal of the fp32 scale, the fp32 product (rounded to 24 bits:
    the double rounding is part of the contract), the clamp, then E4M3 by
    round-to-nearest-even with subnormals (quantum 2^-9) and the zero's sign."""
    sb = int(np.float32(scale).view(np.uint32))
    se, sf = (sb >> 23) & 0xff, sb & 0x7fffff
    assert sb >> 31 == 0 and 0 < se < 255, "a positive normal scale"
    ms, es = (1 << 23) | sf, se - 150                     # s = ms * 2^es
    q, rem = divmod(1 << 60, ms)                          # 1/s = (2^60 / ms) * 2^(-60 - es)
    mr, sh = _rne_scalar(q, rem != 0, 24)
    er = -60 - es + sh                                    # fl32(1/s) = mr * 2^er

    b = bits.astype(np.int64)
    sign = b >> 15
    if dtype is torch.float16:
        e, f, emax, hidden, bias = (b >> 10) & 31, b & 1023, 31, 1024, 25
    else:
        e, f, emax, hidden, bias = (b >> 7) & 255, b & 127, 255, 128, 134
    is_nan = (e == emax) & (f != 0)
    is_inf = (e == emax) & (f == 0)
    mx = np.where(e == 0, f, f + hidden)                  # |x| = mx * 2^ex
    ex = np.where(e == 0, 1, e) - bias

    # fp32 product: 24 significant bits, nearest even (an fp32-subnormal or
    # overflowing product needs no model: it is far below 2^-10 / above 448)
    p = mx * mr
    pe = ex + er
    over = np.maximum(_bit_length(p) - 24, 0)
    m = np.where(over > 0, _rne_shift(p, np.maximum(over, 1)), p)
    me = pe + over
    # exponent of the leading bit; m == 2^24 after a carry is handled by it too
    top = _bit_length(m) - 1 + me
    # clamp to 448 = 0x1.cp8
    norm = np.where(m > 0, m << np.clip(24 - _bit_length(m), 0, 24), 0)   # >= 24 bits, leading bit set
    norm = np.where(_bit_length(norm) > 24, norm >> 1, norm)
    big = (top > 8) | ((top == 8) & (norm >= 0xE00000)) | is_inf
    # E4M3: quantum 2^(max(top, -6) - 3)
    eeff = np.maximum(top, -6)
    shift = (eeff - 3) - me
    k = np.where(shift > 0, _rne_shift(m, np.maximum(shift, 1)), m << np.clip(-shift, 0, 8))
    byte = ((eeff + 6) << 3) + k
    byte = np.where(m == 0, 0, byte)
    byte = np.where(big, 0x7e, byte)
    byte = np.where(is_nan, 0x7f, byte) | (sign << 7)
    return byte.astype(np.uint8), is_nan


def all_patterns(dtype):
    """Every bit pattern of the 16-bit type once, as a CPU tensor."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
