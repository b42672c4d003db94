// Stand-alone check of the packed-weight formats (csrc/pack.hpp and the packers in conv.hpp, conv_tt.hpp, head.hpp, bblockx3.hpp,
// bneckx3.hpp), meant for a sanitizer build on a machine without a GPU (tools/dev/README.md).  Weights, scale and shift come from a fixed
// LCG; every shape is the smallest at which its packer's index arithmetic can go wrong.  Per shape: the packed vector has exactly
// ..._packed_bytes() bytes (the descriptor range the launch hands the kernel), and the FNV-1a hash over the bytes of everything the
// packer produced, in upload order, equals a constant RECORDED FROM THE PACKERS THIS FILE'S COMMIT REPLACED (the ones that lived in
// hrnet_weights.cpp, run on the same generated weights): the move into the kernels' headers changed no byte.  The constants of the
// split (x3) formats hold for the default build (fp16 halves) only; with -DSNCAL_X3_F16=0 those cases check sizes and run the packers
// under the sanitizers, their hashes are printed and not compared.  Nothing here touches a device.
#include "../../soccernet-calibration-sportlight_amd/csrc/conv.hpp"
#include "../../soccernet-calibration-sportlight_amd/csrc/conv_tt.hpp"
#include "../../soccernet-calibration-sportlight_amd/csrc/head.hpp"
#include "../../soccernet-calibration-sportlight_amd/csrc/bblockx3.hpp"
#include "../../soccernet-calibration-sportlight_amd/csrc/bneckx3.hpp"
#include <cstdio>

using namespace sncal;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

struct Layer {
    std::vector<float> w, scale, shift;
    int cout, cin, k;
    Folded folded() const { return Folded{w.data(), scale.data(), cout, cin, k}; }
};
// products of three uniform numbers: weights over several binades, so that the 8- and 16-bit codes meet their subnormals too
static Layer gen(int cout, int cin, int k, uint32_t seed) {
    uint32_t s = seed;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 8388608.f - 1.f; };      // [-1, 1)
    Layer L;
    L.cout = cout; L.cin = cin; L.k = k;
    L.w.resize((size_t)cout * cin * k * k); L.scale.resize(cout); L.shift.resize(cout);
    for (float& v : L.w) { const float a = rnd(), b = rnd(), c = rnd(); v = 0.5f * a * b * c; }
    for (float& v : L.scale) v = 1.f + 0.5f * rnd();
    for (float& v : L.shift) v = 0.1f * rnd();
    return L;
}

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    template <class T> Fnv& add(const std::vector<T>& v) {
        const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
        for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= b[i]; h *= 1099511628211ull; }
        return *this;
    }
};
static void expect(const char* what, uint64_t got, uint64_t want, bool x3 = false) {
    if (x3 && !SNCAL_X3_F16) { printf("%-28s %016llx (bf16 halves: not pinned)\n", what, (unsigned long long)got); return; }
    if (got != want) { printf("FAILED %-28s %016llx, recorded %016llx\n", what, (unsigned long long)got, (unsigned long long)want); ++fails; }
}
template <class T> static size_t bytes(const std::vector<T>& v) { return v.size() * sizeof(T); }

int main() {
    // ---- generic packing (conv.hpp), each shape in the three element forms: bf16 (GE 8), fp32, x3 as [4 hi | 4 lo] (GE 4) ----
    struct { const char* name; int cin, cin_phys, cout, ks, mi, g; uint64_t want[3]; } const generic[] = {
        // Cin below one k-group, taps share k-steps
        {"generic 3x3 3->64", 3, 3, 64, 3, 4, 1, {0x56d5ccc1a946b20eull, 0xd9b91723e20f8972ull, 0x1f587d5a06b8eb51ull}},
        // 54 -> 56 k-groups (bf16): mixed-tap k-steps and a padded last step
        {"generic 3x3 48->48", 48, 48, 48, 3, 3, 6, {0x738a5e6ce5ae69dbull, 0xa5d84bb16d6ceffdull, 0x746a3ad0f7b9c2cdull}},
        // Cout no multiple of MI * 16, Cin below cin_phys
        {"generic 3x3 18->36 in 24", 18, 24, 36, 3, 2, 4, {0xc282f83f188be474ull, 0xfdfa107aa3b033a1ull, 0xdea7e91697b6b899ull}},
        {"generic 1x1 256->64", 256, 256, 64, 1, 4, 8, {0x7db7f5fe7db44ff0ull, 0xad7a6d0ca0c29d43ull, 0xb05b65acc6a1b53eull}},
    };
    uint32_t seed = 1;
    for (const auto& c : generic) {
        const Layer L = gen(c.cout, c.cin, c.ks, seed++);
        for (int form = 0; form < 3; ++form) {
            const ConvPackShape s{c.cin, c.cin_phys, c.cout, c.ks, form == CONV_PACK_BF16 ? 8 : 4, c.mi, c.g};
            std::vector<uint8_t> w;
            std::vector<float> bias;
            conv_pack_weights(L.folded(), L.shift.data(), s, (ConvForm)form, w, bias);
            CHECK(bytes(w) == conv_packed_bytes(s) && bias.size() == (size_t)s.nblk() * c.mi * 16);
            char what[64];
            snprintf(what, sizeof what, "%s %s", c.name, form == 0 ? "bf16" : form == 1 ? "fp32" : "x3");
            expect(what, Fnv().add(w).add(bias).h, c.want[form], form == CONV_PACK_X3);
        }
    }
    // ---- two-team packings (conv_tt.hpp) ----
    struct { const char* name; int cin, cout; uint64_t want; } const tt[] = {
        {"tt bf16 32->96", 32, 96, 0x3eca360545e57526ull},       // one block, one chunk
        {"tt bf16 64->192", 64, 192, 0x59ee9a6384078e8cull},     // block and chunk strides
    };
    for (const auto& c : tt) {
        const Layer L = gen(c.cout, c.cin, 3, seed++);
        CHECK(tt_shape_ok(3, 1, c.cin, c.cin, c.cout));
        std::vector<uint16_t> w;
        tt_pack_weights(L.folded(), w);
        CHECK(bytes(w) == tt_packed_bytes(c.cin, c.cout));
        expect(c.name, Fnv().add(w).h, c.want);
    }
    {   // e4m3: two 64-channel chunks, the second half empty; the weight scales are an output of the packer
        const Layer L = gen(96, 96, 3, seed++);
        std::vector<uint8_t> w;
        std::vector<float> wscale;
        tt8_pack_weights(L.folded(), w, wscale);
        CHECK(bytes(w) == tt8_packed_bytes(96, 96) && wscale.size() == 96);
        expect("tt e4m3 96->96 + wscale", Fnv().add(w).add(wscale).h, 0x38e700b0c05ab5a9ull);
    }
    struct { const char* name; int c, blk; uint64_t want; } const ttx3[] = {
        {"tt x3 48->48", 48, 64, 0x232cf8249b09ac30ull},         // one padded 64-channel block: zero rows above 48
        {"tt x3 96->96", 96, 96, 0x71118267ce8c80c8ull},
    };
    for (const auto& c : ttx3) {
        const Layer L = gen(c.c, c.c, 3, seed++);
        CHECK(x3_shape_ok(3, 1, 2, c.c, c.c, c.c) && ttx3_block(c.c) == c.blk);
        std::vector<uint16_t> w;
        ttx3_pack_weights(L.folded(), c.blk, w);
        CHECK(bytes(w) == ttx3_packed_bytes(c.c, c.c, c.blk));
        expect(c.name, Fnv().add(w).h, c.want, true);
    }
    // ---- fused kernels (bblockx3.hpp, bneckx3.hpp) ----
    {
        const Layer L = gen(48, 48, 3, seed++);
        std::vector<uint16_t> w;
        bbx3_pack_weights(L.folded(), w);
        CHECK(bytes(w) == bbx3_packed_bytes());
        expect("bbx3 48->48", Fnv().add(w).h, 0xd0d697c59ac00494ull, true);
    }
    struct { const char* name; int cin, cout; uint64_t want; } const bnp[] = {
        {"bnp 64->256", 64, 256, 0xee8ec7c781c74198ull},
        {"bnp 256->64", 256, 64, 0x07c4f18cff521186ull},
    };
    for (const auto& c : bnp) {
        const Layer L = gen(c.cout, c.cin, 1, seed++);
        CHECK(bnp_shape_ok(1, 1, c.cin, c.cout));
        std::vector<uint16_t> w;
        bnp_pack_weights(L.folded(), w);
        CHECK(bytes(w) == bnp_packed_bytes(c.cin, c.cout) && bytes(w) == (size_t)BNP_W_BYTES);
        expect(c.name, Fnv().add(w).h, c.want, true);
    }
    // ---- head (head.hpp): last_layer.0 (C -> C) and last_layer.3 (C -> classes) ----
    struct { const char* name; int C, classes; HeadPackShape s; bool split; uint64_t want; } const head[] = {
        // W48, upscale 2: 64 stem + 48 + 96 folded columns = K1 208 (13 k-steps of 16, 7 of 32), 784 -> 800 hidden channels, 58 classes
        {"head W48 bf16", 784, 58, {800, 4, 64, 0, 208, 7}, false, 0xd71de026f8ee064full},
        {"head W48 x3", 784, 58, {800, 4, 64, 0, 208, 7}, true, 0xad29a3bdb52fa1c4ull},
        // K1 = 88 is no multiple of 16: only the 16x16x32 packing exists; 120 -> 128 hidden channels, 23 classes
        {"head K1 88 bf16", 120, 23, {128, 2, 64, 0, 88, 5}, false, 0x4df6397585a7e200ull},
    };
    for (const auto& c : head) {
        const Layer H0 = gen(c.C, c.C, 1, seed++), H1 = gen(c.classes, c.C, 1, seed++);
        CHECK(head_shape_ok(c.s));
        Fnv h;                                     // in upload order: 32x32x16 (hi, then lo), 16x16x32, biases
        if (c.s.K1 % 16 == 0) {
            std::vector<uint16_t> w0, w1, w0_lo, w1_lo;
            head32_pack_weights(H0.folded(), H1.folded(), c.s, c.split, w0, w1, w0_lo, w1_lo);
            CHECK(bytes(w0) == head32_w0_packed_bytes(c.s) && bytes(w1) == head32_w1_packed_bytes(c.s));
            CHECK(bytes(w0_lo) == (c.split ? bytes(w0) : 0) && bytes(w1_lo) == (c.split ? bytes(w1) : 0));
            h.add(w0).add(w1).add(w0_lo).add(w1_lo);
        }
        if (!c.split) {
            std::vector<uint16_t> w0, w1;
            head_pack_weights(H0.folded(), H1.folded(), c.s, w0, w1);
            CHECK(bytes(w0) == head_w0_packed_bytes(c.s) && bytes(w1) == head_w1_packed_bytes(c.s));
            h.add(w0).add(w1);
        }
        std::vector<float> b0, b1;
        head_pack_bias(H0.shift.data(), H0.cout, H1.shift.data(), H1.cout, c.s, b0, b1);
        CHECK(b0.size() == (size_t)c.s.HP && b1.size() == 64);
        expect(c.name, h.add(b0).add(b1).h, c.want, c.split);
    }
    // ---- the scalar converters (pack.hpp) at their edges ----
    CHECK(f2bf(1.f) == 0x3f80 && f2bf(1.00390625f) == 0x3f80 && f2bf(1.01171875f) == 0x3f82 && f2bf(-0.f) == 0x8000);      // ties to even
    CHECK(f2fp8(448.f) == 0x7e && f2fp8(1e9f) == 0x7e && f2fp8(-1e9f) == 0xfe && f2fp8(0.f) == 0 && f2fp8(1.f) == 0x38);
    CHECK(f2fp8(0.001953125f) == 0x01 && f2fp8(0.0009765625f) == 0x00 && f2fp8(0.015625f) == 0x08);      // 2^-9, half of it, smallest normal
    // f2h / h2f against the compiler's own conversions: every half, and every 4099th float (all exponents, both signs, NaNs; the full
    // 2^32 sweep is profiles/pack_frame.md's)
    int cast_diffs = 0;
    for (uint32_t c = 0; c < 65536; ++c) {
        const uint16_t code = (uint16_t)c;
        _Float16 h;
        memcpy(&h, &code, 2);
        const float want = (float)h, got = h2f(code);
        cast_diffs += memcmp(&want, &got, 4) != 0;
    }
    for (uint64_t u = 0; u < (1ull << 32); u += 4099) {
        const uint32_t bits = (uint32_t)u;
        float f;
        memcpy(&f, &bits, 4);
        const _Float16 h = (_Float16)f;
        uint16_t want;
        memcpy(&want, &h, 2);
        cast_diffs += want != f2h(f);
    }
    CHECK(cast_diffs == 0);
    CHECK(f2h(65504.f) == 0x7bff && f2h(65519.996f) == 0x7bff && f2h(65520.f) == 0x7c00 && f2h(-65520.f) == 0xfc00);      // the tie above the largest half
    CHECK(f2h(6.103515625e-05f) == 0x0400 && f2h(2.98023223876953125e-08f) == 0 && f2h(2.9802325940409414e-08f) == 1);  // 2^-14; 2^-25 ties to zero
    uint32_t seen = 0;
    for (int r = 0; r < 32; ++r) seen |= 1u << h32_row_channel(r);
    CHECK(seen == 0xffffffffu);                            // a permutation of 0..31
    printf(fails ? "pack_host_check: %d FAILED\n" : "pack_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
