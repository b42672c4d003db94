"""CPU: the references of the twin hand-offs (tests/handoff_ref.py split16 / e4m3_codes, used without a tolerance by the GPU tests) against
an independent bit-level round-to-nearest-even (handoff_ref.rne_codes: exact float64 arithmetic on the value, no conversion of torch's
or numpy's involved) -- on every finite bf16 value, the fp16 clamp boundary, subnormals, signed zeros and exact ties of both formats."""
import numpy as np
import pytest
import torch

import handoff_ref as hr


def _all_finite_bf16():
    codes = np.arange(65536, dtype=np.int64)
    codes = codes[((codes >> 7) & 0xff) != 0xff]                          # no infinities / NaNs
    assert codes.size == 65280
    return (codes.astype(np.uint32) << 16).view(np.float32)


def _pad16(v):
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    return np.concatenate([v, np.zeros((-v.size) % 16, dtype=np.float32)]).reshape(-1, 16)


def _edge_values(dtype):
    ebits, mbits = hr.FORMATS[dtype]
    bias = 2 ** (ebits - 1) - 1
    v = [0.0, -0.0, 1.0, -1.0, 65504.0, 65520.0, 65519.99, 65536.0, 1e6, -1e6, -65504.0, -65520.0, 3.0e38, -3.0e38,
         2.0 ** -149, 2.0 ** -126, -2.0 ** -126]
    sub = 2.0 ** (1 - bias - mbits)                                       # the format's smallest subnormal
    v += [sub, -sub, 0.5 * sub, -0.5 * sub, 0.5 * sub * (1 + 2.0 ** -20), 1.5 * sub, 2.5 * sub, 0.25 * sub, (2 ** mbits - 0.5) * sub,
          (2 ** mbits - 1) * sub, 2.0 ** (1 - bias), 2.0 ** (1 - bias) * (1 - 2.0 ** -12)]
    for e in (-20, -14, -3, 0, 7, 15):                                    # exact ties of the hi rounding: odd and even neighbours
        ulp = 2.0 ** (e - mbits)
        for k in (0, 1, 2, 3, 2 ** mbits - 1):
            v += [2.0 ** e + (k + 0.5) * ulp, -(2.0 ** e + (k + 0.5) * ulp), 2.0 ** e + (k + 0.5) * ulp * (1 + 2.0 ** -10)]
            # ... and of the lo rounding: x = hi + (odd + 1/2) ulp(lo)
            v += [2.0 ** e + k * ulp + (2 * k + 1.5) * ulp * 2.0 ** -(mbits + 2)]
    return np.asarray(v, dtype=np.float32)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_split16_is_the_bit_level_split(dtype):
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2 ** 32, size=1 << 18, dtype=np.uint64).astype(np.uint32)
    rand = bits.view(np.float32)
    rand = rand[np.isfinite(rand)]
    wide = (rng.standard_normal(1 << 16) * np.exp(rng.uniform(-12, 12, 1 << 16))).astype(np.float32)       # the activations' range
    for name, vals in (('edges', _edge_values(dtype)), ('all finite bf16', _all_finite_bf16()), ('random bits', rand), ('wide normal', wide)):
        x = _pad16(vals)
        if dtype == torch.bfloat16:                          # no clamp in the bf16 build: values whose hi would round to infinity are not its business
            x = np.where(np.abs(x) < np.float32(3.3e38), x, np.float32(0))
        got = hr.split16(torch.from_numpy(x), dtype).numpy().astype(np.int64) & 0xffff
        want = hr.split16_bits(x, dtype)
        assert got.shape == want.shape == (x.shape[0], 32)
        bad = got != want
        assert not bad.any(), f'{name}: {int(bad.sum())} codes differ, first at {np.argwhere(bad)[0]}: x = {x[np.argwhere(bad)[0][0]]}'
    # the layout: per 16 channels the hi codes, then the lo codes
    x = (np.arange(32, dtype=np.float32) + 1.0) * np.float32(1.0 + 2.0 ** -12)
    c = hr.split16(torch.from_numpy(x[None]), dtype).view(dtype).to(torch.float32).numpy()[0]
    for g in range(2):
        hi, lo = c[32 * g:32 * g + 16], c[32 * g + 16:32 * g + 32]
        assert np.array_equal(hi, torch.from_numpy(x[16 * g:16 * g + 16]).to(dtype).to(torch.float32).numpy())
        assert np.all(lo != 0) and np.allclose(hi + lo, x[16 * g:16 * g + 16], rtol=2.0 ** -15, atol=0)
    if dtype == torch.float16:                               # the clamp: both parts finite, hi = +-65504, lo = 0
        c = hr.split16(torch.tensor([[65520.0, -1e6] + [0.0] * 14]), dtype).view(dtype)[0]
        assert c[0] == 65504 and c[1] == -65504 and c[16] == 0 and c[17] == 0


def test_e4m3_codes_is_the_bit_level_quantiser():
    x = _all_finite_bf16()
    xt = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(xt.to(torch.float32).numpy(), x)
    amax = float(np.abs(x).max())
    # a calibrated scale (amax / 448), ordinary ones, one that saturates most of the range, one that pushes everything into subnormals
    for scale in (np.float32(amax) / np.float32(448.0), np.float32(1.0), np.float32(0.0123), np.float32(3.7), np.float32(2.0 ** -20), np.float32(1e-30),
                  np.float32(2.0 ** 100)):
        got = hr.e4m3_codes(xt, float(scale)).numpy().astype(np.int64)
        want = hr.e4m3_bits(x, scale)
        assert (want & 0x7f).max() <= 0x7e                                   # saturated: no NaN encoding
        dv = hr.e4m3_values(torch.from_numpy(got.astype(np.uint8))).numpy().astype(np.float64)
        assert np.array_equal(dv, hr.code_values(want, 4, 3)), f'scale {scale}: {int((dv != hr.code_values(want, 4, 3)).sum())} values differ'
        assert np.array_equal(got, want), f'scale {scale}: codes differ (signed zeros included)'
    # exact ties of e4m3 at scale 1 (bf16 holds them: 4 significand bits needed), subnormal ties, the saturation edge
    ties = np.asarray([1.0625, 1.1875, -1.0625, 17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11, 448.0, 464.0, 480.0, -1e9, 0.0, -0.0], dtype=np.float32)
    got = hr.e4m3_values(hr.e4m3_codes(torch.from_numpy(ties).to(torch.bfloat16), 1.0)).numpy()
    assert np.array_equal(got, np.asarray([1.0, 1.25, -1.0, 16.0, 20.0, 0.0, 2.0 ** -8, 0.0, 448.0, 448.0, 448.0, -448.0, 0.0, 0.0], dtype=np.float32)), got
    # 1.0f / scale is formed in fp32: for this scale the fp64 reciprocal rounds a product to the other neighbour somewhere
    assert hr.inv_scale(3.0) == float(np.float32(1.0) / np.float32(3.0)) != 1.0 / 3.0


def test_rne_codes_against_hand_values():
    """The independent side itself, on values worked out by hand."""
    f16 = lambda v: int(hr.rne_codes(np.float32(v), 5, 10))
    assert f16(1.0) == 0x3c00 and f16(-2.0) == 0xc000 and f16(65504.0) == 0x7bff and f16(0.0) == 0 and f16(-0.0) == 0x8000
    assert f16(2.0 ** -24) == 1 and f16(2.0 ** -25) == 0 and f16(1.5 * 2.0 ** -24) == 2 and f16(2.0 ** -14) == 0x0400
    assert f16(1.0 + 2.0 ** -11) == 0x3c00 and f16(1.0 + 3 * 2.0 ** -11) == 0x3c02 and f16(2.0 - 2.0 ** -12) == 0x4000
    bf = lambda v: int(hr.rne_codes(np.float32(v), 8, 7))
    assert bf(1.0) == 0x3f80 and bf(1.0 + 2.0 ** -8) == 0x3f80 and bf(1.0 + 3 * 2.0 ** -8) == 0x3f82 and bf(-3.0) == 0xc040
    e4 = lambda v: int(hr.rne_codes(np.float32(v), 4, 3))
    assert e4(448.0) == 0x7e and e4(1.0) == 0x38 and e4(2.0 ** -9) == 1 and e4(2.0 ** -6) == 0x08 and e4(-0.0) == 0x80
    assert float(hr.code_values(0x7e, 4, 3)) == 448.0 and float(hr.code_values(0x7bff, 5, 10)) == 65504.0 and float(hr.code_values(1, 5, 10)) == 2.0 ** -24
