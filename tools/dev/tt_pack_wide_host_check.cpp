// Stand-alone check of the two-team kernel's three weight packers (csrc/conv_tt.hpp) at widths no packaged config has, meant for a
// sanitizer build on a machine without a GPU (tools/dev/README.md).  pack_host_check.cpp pins the BYTES of the packers at the smallest
// shapes; this one checks the MEANING of every element against the layout comment above each packer, at the widths where the block and
// chunk arithmetic has remainders:
//
//   ttx3_pack_weights   (cin, cout, blk) = (80, 80, 64) a partial last block of 16 behind a full one, 5 chunks; (176, 176, 64) the 48-channel
//                       last block at nb = 2, 11 chunks; (400, 400, 64) 6 full blocks + 16, 25 chunks; (288, 288, 96), (480, 480, 96)
//   tt_pack_weights     288 -> 288 and 480 -> 480: 3 and 5 blocks of 96, 9 and 15 chunks of 32
//   tt8_pack_weights    the same two: ceil(cin / 64) = 5 and 8 chunks, the last one half empty
//
// W lives in a heap buffer of EXACTLY cout * cin * 9 floats (scale: cout), so AddressSanitizer reports a packer that reads a row at or above
// cout or a channel at or above cin.  Per case: the vector has ..._packed_bytes() bytes; every real (co, ci, tap) sits at the index the
// layout comment gives (computed here from the comment, not from the packer's loop) and holds the right value -- split engine: hi + lo equals
// the folded weight to the split's precision and hi is its rounding; bf16: f2bf of it; e4m3: f2fp8 of it over the channel's scale --; every
// other element (rows at or above cout, e4m3 slots at or above cin) is zero.  Nothing here touches a device.
#include "../../soccernet-calibration-sportlight_amd/csrc/conv_tt.hpp"
#include <cmath>
#include <cstdio>
#include <memory>

using namespace sncal;

static int fails = 0;
static const char* case_name = "";
#define CHECK(c) do { if (!(c)) { if (fails < 40) printf("FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, case_name, #c); ++fails; } } while (0)

struct Layer {
    std::unique_ptr<float[]> w, scale;          // exactly cout * cin * 9 and cout floats
    int cout, cin;
    Folded folded() const { return Folded{w.get(), scale.get(), cout, cin, 3}; }
    float value(int co, int ci, int t) const { return w[((size_t)co * cin + ci) * 9 + t] * scale[co]; }
};
// products of three uniform numbers: weights over several binades (pack_host_check.cpp's generator)
static Layer gen(int cout, int cin, uint32_t seed) {
    uint32_t s = seed;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 8388608.f - 1.f; };
    Layer L;
    L.cout = cout; L.cin = cin;
    const size_t n = (size_t)cout * cin * 9;
    L.w.reset(new float[n]); L.scale.reset(new float[cout]);
    for (size_t i = 0; i < n; ++i) { const float a = rnd(), b = rnd(), c = rnd(); L.w[i] = 0.5f * a * b * c; }
    for (int i = 0; i < cout; ++i) L.scale[i] = 1.f + 0.5f * rnd();
    return L;
}

// MFMA row of a 32-row block that carries channel ch of the block (the inverse of pack.hpp h32_row_channel)
static int row_of_channel(int ch) {
    for (int r = 0; r < 32; ++r) if (h32_row_channel(r) == ch) return r;
    return -1;
}

// split engine: a layer = [nb][c] stages of [tap 9][part: hi, lo][32-row block MB][lane 64] x 8 codes; lane l holds output channel
// nb * blk + mb * 32 + h32_row_channel(l & 31), input channels c * 16 + (l >> 5) * 8 + 0..7
static void check_x3(int cin, int cout, int blk, uint32_t seed) {
    static char name[64];
    snprintf(name, sizeof name, "x3 %d->%d blk %d", cin, cout, blk);
    case_name = name;
    const Layer L = gen(cout, cin, seed);
    CHECK(x3_shape_ok(3, 1, 2, cin, cin, cout) && ttx3_block(cout) == blk);
    std::vector<uint16_t> out;
    ttx3_pack_weights(L.folded(), blk, out);
    CHECK(out.size() * 2 == ttx3_packed_bytes(cin, cout, blk));
    const int MBk = blk / 32, chunks = cin / 16, nblk = (cout + blk - 1) / blk;
    CHECK(out.size() == (size_t)nblk * chunks * 9 * 2 * MBk * 64 * 8);
    std::vector<uint8_t> real(out.size(), 0);
    size_t n_real = 0;
    double worst = 0;
    for (int co = 0; co < cout; ++co) {
        const int nb = co / blk, mb = co % blk / 32, row = row_of_channel(co % 32);
        for (int ci = 0; ci < cin; ++ci) {
            const int c = ci / 16, lane = row + 32 * (ci % 16 / 8), e = ci % 8;
            for (int t = 0; t < 9; ++t) {
                const size_t ih = ((((((size_t)nb * chunks + c) * 9 + t) * 2 + 0) * MBk + mb) * 64 + lane) * 8 + e;
                const size_t il = ((((((size_t)nb * chunks + c) * 9 + t) * 2 + 1) * MBk + mb) * 64 + lane) * 8 + e;
                if (ih >= out.size() || il >= out.size()) { CHECK(!"index inside the vector"); continue; }
                real[ih] = real[il] = 1;
                n_real += 2;
                const float w = L.value(co, ci, t), hi = x3_value_host(out[ih]), lo = x3_value_host(out[il]);
                // hi is the 16-bit rounding of w, lo of the remainder: fp16 halves 2^-22 |w| (+ 2^-25 where lo is subnormal), bf16 2^-16 |w|
                const double tol = SNCAL_X3_F16 ? std::ldexp(std::fabs((double)w), -21) + std::ldexp(1.0, -24) : std::ldexp(std::fabs((double)w), -15);
                const double err = std::fabs((double)hi + (double)lo - (double)w);
                worst = std::max(worst, err / tol);
                CHECK(err <= tol);
                CHECK(out[ih] == x3_code_host(w));
            }
        }
    }
    CHECK(n_real == (size_t)cout * cin * 9 * 2);
    size_t zeros = 0;
    for (size_t i = 0; i < out.size(); ++i)
        if (!real[i]) { CHECK(out[i] == 0); ++zeros; }
    CHECK(zeros == (size_t)(nblk * blk - cout) * cin * 9 * 2);        // the rows at or above cout, nothing else
    printf("%-24s %8zu codes, %7zu zero rows' codes, worst |hi + lo - w| / tol %.3f\n", name, out.size(), zeros, worst);
}

// bf16: a layer = [nb][c] stages of [tap 9][channel half 2][32-row block 3][lane 64] x 8 bf16; lane l holds output channel
// nb * 96 + mb * 32 + (l & 31), input channels c * 32 + h * 16 + (l >> 5) * 8 + 0..7
static void check_bf16(int cin, int cout, uint32_t seed) {
    static char name[64];
    snprintf(name, sizeof name, "bf16 %d->%d", cin, cout);
    case_name = name;
    const Layer L = gen(cout, cin, seed);
    CHECK(tt_shape_ok(3, 1, cin, cin, cout));
    std::vector<uint16_t> out;
    tt_pack_weights(L.folded(), out);
    CHECK(out.size() * 2 == tt_packed_bytes(cin, cout));
    const int chunks = cin / 32;
    CHECK(out.size() == (size_t)(cout / 96) * chunks * 9 * 2 * 3 * 64 * 8);
    std::vector<uint8_t> real(out.size(), 0);
    for (int co = 0; co < cout; ++co) {
        const int nb = co / 96, mb = co % 96 / 32;
        for (int ci = 0; ci < cin; ++ci) {
            const int c = ci / 32, h = ci % 32 / 16, lane = co % 32 + 32 * (ci % 16 / 8), e = ci % 8;
            for (int t = 0; t < 9; ++t) {
                const size_t i = ((((((size_t)nb * chunks + c) * 9 + t) * 2 + h) * 3 + mb) * 64 + lane) * 8 + e;
                if (i >= out.size()) { CHECK(!"index inside the vector"); continue; }
                CHECK(!real[i]);
                real[i] = 1;
                CHECK(out[i] == f2bf(L.value(co, ci, t)));
            }
        }
    }
    size_t unreal = 0;
    for (size_t i = 0; i < out.size(); ++i) unreal += !real[i];
    CHECK(unreal == 0);                                                // cout % 96 == 0 and cin % 32 == 0: no padding at all
    printf("%-24s %8zu codes, every one a real weight\n", name, out.size());
}

// e4m3: a layer = [nb][c] stages of [tap 9][32-row block 3][half 2][lane 64] x 16 codes, 64-channel chunks; lane l holds output channel
// nb * 96 + mb * 32 + (l & 31), input channels c * 64 + 32 (l >> 5) + 16 half + 0..15 (zeros beyond cin); wscale = max |w| / 448
static void check_fp8(int cin, int cout, uint32_t seed) {
    static char name[64];
    snprintf(name, sizeof name, "e4m3 %d->%d", cin, cout);
    case_name = name;
    const Layer L = gen(cout, cin, seed);
    std::vector<uint8_t> out;
    std::vector<float> ws;
    tt8_pack_weights(L.folded(), out, ws);
    CHECK(out.size() == tt8_packed_bytes(cin, cout) && (int)ws.size() == cout);
    const int chunks = (cin + 63) / 64;
    CHECK(out.size() == (size_t)(cout / 96) * chunks * 9 * 3 * 2 * 64 * 16);
    std::vector<uint8_t> real(out.size(), 0);
    for (int co = 0; co < cout; ++co) {
        float mx = 0.f;
        for (int ci = 0; ci < cin; ++ci) for (int t = 0; t < 9; ++t) mx = std::max(mx, std::fabs(L.value(co, ci, t)));
        CHECK(ws[co] == (mx > 0.f ? mx / 448.f : 1.f));
        const int nb = co / 96, mb = co % 96 / 32;
        for (int ci = 0; ci < cin; ++ci) {
            const int c = ci / 64, lane = co % 32 + 32 * (ci % 64 / 32), half = ci % 32 / 16, e = ci % 16;
            for (int t = 0; t < 9; ++t) {
                const size_t i = ((((((size_t)nb * chunks + c) * 9 + t) * 3 + mb) * 2 + half) * 64 + lane) * 16 + e;
                if (i >= out.size()) { CHECK(!"index inside the vector"); continue; }
                CHECK(!real[i]);
                real[i] = 1;
                CHECK(out[i] == f2fp8(L.value(co, ci, t) / ws[co]));
            }
        }
    }
    size_t zeros = 0;
    for (size_t i = 0; i < out.size(); ++i)
        if (!real[i]) { CHECK(out[i] == 0); ++zeros; }
    CHECK(zeros == (size_t)cout * (chunks * 64 - cin) * 9);             // the slots at or above cin of the last chunk, nothing else
    printf("%-24s %8zu codes, %7zu zero slots beyond cin\n", name, out.size(), zeros);
}

int main() {
    for (int r = 0; r < 32; ++r) CHECK(row_of_channel(h32_row_channel(r)) == r);
    const int x3[][3] = {{80, 80, 64}, {176, 176, 64}, {400, 400, 64}, {288, 288, 96}, {480, 480, 96}};
    uint32_t seed = 101;
    for (const auto& c : x3) check_x3(c[0], c[1], c[2], seed++);
    for (int c : {288, 480}) check_bf16(c, c, seed++);
    for (int c : {288, 480}) check_fp8(c, c, seed++);
    printf(fails ? "tt_pack_wide_host_check: %d FAILED\n" : "tt_pack_wide_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
