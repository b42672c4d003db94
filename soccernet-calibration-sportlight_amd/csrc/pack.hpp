// What the weight packers share.  A packed-weight format is a byte layout that ONE kernel reads through a buffer descriptor; it is owned
// by that kernel's header (conv.hpp, conv_tt.hpp, head.hpp, bblockx3.hpp, bneckx3.hpp): a pure host function that fills a std::vector
// from folded weights and plain integers, and beside it the ..._packed_bytes() with which the packer sizes its vector -- the number the
// launch hands the kernel as its descriptor range (DevBuf::bytes, hrnet_net.hpp).  Here: the scalar converters to the 16- and 8-bit
// storage formats, the accessor of a folded weight, the row order of a 32-row MFMA fragment.  Host only, no HIP call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace sncal {

inline uint16_t f2bf(float f) {   // float -> bf16, round to nearest even
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// float -> IEEE binary16 and back, round to nearest even: bit for bit what the casts to and from _Float16 give.  On a host without a
// half-precision instruction the casts are calls into the compiler's soft-float library, three per weight in the split packers' element
// loops, which were most of a model's load time; these inline
inline uint16_t f2h(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return sign | 0x7e00 | (uint16_t)((u >> 13) & 0x1ffu);      // NaN: quiet, payload kept
    if (u >= 0x477ff000u) return sign | 0x7c00;                                       // 65520 (the tie above 65504) and up: infinity
    if (u >= 0x38800000u) {                                                           // normal half: rebias, round the 13 dropped bits
        u -= 0x38000000u;
        u += 0xfffu + ((u >> 13) & 1u);
        return sign | (uint16_t)(u >> 13);
    }
    float a;                                               // below 2^-14: a + 0.5 has an ulp of 2^-24, the subnormal halves' spacing, so
    memcpy(&a, &u, 4);                                     // the adder rounds to it (nearest even) and leaves the code in the low bits
    a += 0.5f;
    memcpy(&u, &a, 4);
    return sign | (uint16_t)(u - 0x3f000000u);
}
inline float h2f(uint16_t c) {
    const uint32_t sign = (uint32_t)(c & 0x8000u) << 16, e = (c >> 10) & 31u, m = c & 0x3ffu;
    uint32_t u;
    if (e == 0) {                                          // zero and subnormals: m * 2^-24, exact
        const float a = (float)m * 5.9604644775390625e-08f;
        memcpy(&u, &a, 4);
        u |= sign;
    }
    else u = sign | ((e == 31 ? 255u : e + 112u) << 23) | (m << 13);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// float -> OCP e4m3fn (1-4-3, bias 7, max 448, no infinities), round to nearest even, saturating
inline uint8_t f2fp8(float f) {
    if (!(f == f)) return 0x7f;
    const uint8_t sign = f < 0 ? 0x80 : 0;
    float a = std::fabs(f);
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0.0009765625f) return sign;                    // below half the smallest subnormal (2^-9 / 2): zero
    int e;
    float m = std::frexp(a, &e);                            // a = m * 2^e, m in [0.5, 1)
    int E = e - 1 + 7;                                      // biased exponent of 1.xxx * 2^(e-1)
    int q;
    if (E >= 1) {                                           // normal: 3 mantissa bits
        const float x = (m * 2.f - 1.f) * 8.f;
        q = (int)std::nearbyint(x);
        if (q == 8) { q = 0; ++E; }
        if (E > 15 || (E == 15 && q > 6)) return sign | 0x7e;
        return sign | (uint8_t)(E << 3) | (uint8_t)q;
    }
    q = (int)std::nearbyint(a * 512.f);                     // subnormal: multiples of 2^-9
    if (q >= 8) return sign | 0x08;
    return sign | (uint8_t)q;
}

// The weights of a layer as every packer reads them: w [cout][cin][k][k] with the folded-BN scale [cout] applied.  Packers take it by
// value: their byte stores may alias whatever is reached through a reference, a local copy stays in registers over the loops
struct Folded {
    const float* w;
    const float* scale;
    int cout, cin, k;
    float operator()(int co, int ci, int ky, int kx) const { return w[(((size_t)co * cin + ci) * k + ky) * k + kx] * scale[co]; }
    // the same for a packer whose format fixes the kernel size: tap t = ky * K + kx of a K x K layer
    template <int K> float tap(int co, int ci, int t = 0) const { return w[((size_t)co * cin + ci) * (K * K) + t] * scale[co]; }
    float max_abs(int co) const {      // largest |folded weight| of an output channel (its cin * k * k weights are contiguous)
        const float* row = w + (size_t)co * cin * k * k;
        const float sc = scale[co];
        float mx = 0.f;
        for (size_t i = 0; i < (size_t)cin * k * k; ++i) mx = std::max(mx, std::fabs(row[i] * sc));
        return mx;
    }
};

// Row order of a 32-row block of A fragments of v_mfma_f32_32x32x16 (head32.hip, headx3.hip, bneckx3.hip, conv_tt.hip's x3 mode).  The D
// registers give lane l rows 8 q + 4 (l >> 5) + j (q, j = 0..3) of column l & 31; MFMA row r carries channel h32_row_channel(r) of the
// block, so that the registers 8 h .. 8 h + 7 of a lane are the eight consecutive channels 16 h + 8 (l >> 5) + 0..7.
constexpr int h32_row_channel(int r) { return 16 * (r >> 4) + 8 * ((r >> 2) & 1) + 4 * ((r >> 3) & 1) + (r & 3); }

}  // namespace sncal
