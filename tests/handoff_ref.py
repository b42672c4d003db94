"""The two hand-off conversions of the reduced-precision engines, restated in torch (csrc/quant.hip, csrc/x3.hpp):

    split16(x, dtype)            fp32 (..., C) -> the [16 hi | 16 lo] 16-bit codes of the split twin, (..., 2 C) int16
    e4m3_codes(x_bf16, scale)    bf16 (...)    -> the e4m3 codes of the fp8 twin, (...) uint8

Both are deterministic fp32 + round-to-nearest-even arithmetic, so tests/test_kernels_gpu.py and tests/test_handoff_gpu.py compare the
twins a forward made with them WITHOUT a tolerance; tests/test_handoff_host.py holds the two functions themselves to a bit-level numpy
rounding (rne_codes below) that shares no conversion code with torch."""
import numpy as np
import torch

F16_MAX = 65504.0
E4M3_MAX = 448.0


def split16(x, dtype):
    """hi = rne16(xc), lo = rne16(xc - float(hi)) with xc = clamp(x, +-65504) for fp16 splits and xc = x for bf16 splits (x3.hpp
    X3_SPLIT*); x - hi is exact in fp32.  Per 16-channel group of the last axis the 16 hi codes, then the 16 lo codes."""
    assert x.dtype == torch.float32 and x.shape[-1] % 16 == 0, (x.dtype, tuple(x.shape))
    xc = x.clamp(-F16_MAX, F16_MAX) if dtype == torch.float16 else x
    hi = xc.to(dtype)
    lo = (xc - hi.to(torch.float32)).to(dtype)
    lead, groups = tuple(x.shape[:-1]), x.shape[-1] // 16
    pair = torch.stack((hi.reshape(*lead, groups, 16), lo.reshape(*lead, groups, 16)), dim=-2)         # (..., G, 2, 16)
    return pair.reshape(*lead, 2 * x.shape[-1]).contiguous().view(torch.int16)


def split_codes_of_twin(raw):
    """A tapped split twin (fp32-typed storage, (..., C)) as its (..., 2 C) int16 codes."""
    return raw.contiguous().view(torch.int16)


def inv_scale(scale):
    """1.0f / scale in fp32, as the host forms it (quant.hip launch_quantize_fp8, hrnet.cpp tt_member)."""
    return float(np.float32(1.0) / np.float32(scale))


def e4m3_codes(x_bf16, scale):
    """e4m3_rne(clamp(float(x) * (1.0f / scale), +-448)): the fp32 product is rounded once, saturated, then rounded to e4m3."""
    assert x_bf16.dtype == torch.bfloat16, x_bf16.dtype
    inv = torch.tensor(inv_scale(scale), dtype=torch.float32, device=x_bf16.device)
    v = (x_bf16.to(torch.float32) * inv).clamp(-E4M3_MAX, E4M3_MAX)
    return v.to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(codes):
    return codes.view(torch.float8_e4m3fn).to(torch.float32)


# ---- the independent side: round-to-nearest-even by exact arithmetic on the value, no conversion instruction involved ------------
def rne_codes(x, ebits, mbits):
    """Finite fp32 values -> integer codes of the binary format with `ebits` exponent bits (bias 2^(ebits-1) - 1, gradual underflow)
    and `mbits` stored significand bits, round-to-nearest-even.  In float64 every step is exact: |x| / quantum is an integer plus a
    fraction of at most 24 significant bits, np.rint rounds halves to even.  Values that round beyond the format's exponent range are
    the caller's business (the hand-offs clamp first); the exponent field is returned as it comes out."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x.astype(np.float64))
    bias = 2 ** (ebits - 1) - 1
    _, e = np.frexp(a)                                            # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    E = np.maximum(e.astype(np.int64) - 1, 1 - bias)              # subnormals share the smallest normal exponent
    q = np.rint(a / np.ldexp(1.0, E - mbits))                     # significand in units of the last place
    carry = q >= 2.0 ** (mbits + 1)                               # rounded up to the next power of two
    E = np.where(carry, E + 1, E)
    q = np.where(carry, q / 2.0, q).astype(np.int64)
    normal = q >= 2 ** mbits
    field = np.where(normal, E + bias, 0)
    mant = np.where(normal, q - 2 ** mbits, q)
    return (np.signbit(x).astype(np.int64) << (ebits + mbits)) | (field << mbits) | mant


def code_values(codes, ebits, mbits):
    """The way back, exact in float64."""
    codes = np.asarray(codes, dtype=np.int64)
    bias = 2 ** (ebits - 1) - 1
    field, mant = (codes >> mbits) & (2 ** ebits - 1), codes & (2 ** mbits - 1)
    mag = np.where(field > 0, np.ldexp(1.0 + mant / 2.0 ** mbits, field - bias), np.ldexp(mant / 2.0 ** mbits, 1 - bias))
    return np.where((codes >> (ebits + mbits)) & 1, -mag, mag)


FORMATS = {torch.float16: (5, 10), torch.bfloat16: (8, 7), torch.float8_e4m3fn: (4, 3)}


def split16_bits(x, dtype):
    """split16 on rne_codes: numpy fp32 (..., C) -> (..., 2 C) int64 codes."""
    ebits, mbits = FORMATS[dtype]
    x = np.asarray(x, dtype=np.float32)
    xc = np.clip(x, np.float32(-F16_MAX), np.float32(F16_MAX)) if dtype == torch.float16 else x
    hi = rne_codes(xc, ebits, mbits)
    rest = xc.astype(np.float64) - code_values(hi, ebits, mbits)              # exact, and representable in fp32
    assert np.array_equal(rest.astype(np.float32).astype(np.float64), rest)
    lo = rne_codes(rest.astype(np.float32), ebits, mbits)
    lead, groups = x.shape[:-1], x.shape[-1] // 16
    pair = np.stack((hi.reshape(*lead, groups, 16), lo.reshape(*lead, groups, 16)), axis=-2)
    return pair.reshape(*lead, 2 * x.shape[-1])


def e4m3_bits(x_f32_of_bf16, scale):
    """e4m3_codes on rne_codes: numpy fp32 array holding bf16 values -> int64 codes."""
    inv = np.float32(1.0) / np.float32(scale)
    with np.errstate(over='ignore'):                                          # (an infinite product saturates like any other)
        v = (np.asarray(x_f32_of_bf16, dtype=np.float32) * inv).astype(np.float32)
    v = np.clip(v, np.float32(-E4M3_MAX), np.float32(E4M3_MAX))
    return rne_codes(v, 4, 3)
