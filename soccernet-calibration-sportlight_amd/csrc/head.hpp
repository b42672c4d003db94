// Parameters / launchers of the fused head kernels (head.hip, head32.hip, headx3.hip, headx4.hip; their shared device pieces: head_frame.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "pack.hpp"      // h32_row_channel: the row order of head32.hip's and headx3.hip's 32-row blocks
#include "x3.hpp"        // x3_split_host

namespace sncal {

constexpr int HEAD_MAX_SRC = 5;
constexpr int HEAD_MAX_FOLD = 2;

struct HeadParams {
    const void* direct;            // [N][H][W][Cd] bf16: the tensor that already sits at head resolution
    int Cd;                        // its channel count (<= 64)
    int nfold;                     // narrow branches whose upsampled channels are appended to the stage-1 K dimension
    const void* fold[HEAD_MAX_FOLD];   // [N][Hf][Wf][Cf] bf16
    int Cf[HEAD_MAX_FOLD], Hf[HEAD_MAX_FOLD], Wf[HEAD_MAX_FOLD];
    float fsy[HEAD_MAX_FOLD], fsx[HEAD_MAX_FOLD];
    int ks1;                       // stage-1 k-steps: ceil((Cd + sum Cf) / 32), rounded up to an instantiated depth
    const void* w0;                // stage-1 A fragments [NQ][2][ks1][64 lanes] x 16 B (rows permuted, BN scale folded)
    const float* bias0;            // [HP] folded BN shift of last_layer.0 (zero on the padding)
    const void* w1;                // stage-2 A fragments [NQ][M2][64 lanes] x 16 B
    const void* w0_32;             // head32.hip: stage-1 A fragments of v_mfma_f32_32x32x16 [NQ][ks16][64 lanes] x 16 B (rows in h32_row_channel order), or null
    const void* w1_32;             // head32.hip: stage-2 A fragments [NQ][ceil(LC / 32)][2][64 lanes] x 16 B (class rows in h32_row_channel order)
    const void* w0_32_lo;          // headx3.hip (fp16x3 engine): the lo parts of the split weights, same layouts (w0_32 / w1_32 hold the hi parts)
    const void* w1_32_lo;
    int ks16;                      // (Cd + sum Cf) / 16 when that is exact, else 0
    const float* bias1;            // [LC] bias of last_layer.3 (zero on the padding)
    int nsrc;
    const void* src[HEAD_MAX_SRC]; // t_i = W0_i . branch_i at native resolution, [N][Hs][Ws][HP] bf16
    int Hs[HEAD_MAX_SRC], Ws[HEAD_MAX_SRC];
    float sy[HEAD_MAX_SRC], sx[HEAD_MAX_SRC];
    float* logits;                 // [N][H][W][LC] fp32
    // head32.hip, decode-fused form (nobody wants the heatmap): log-softmax and the tile's row / column maxima in the epilogue, no logits
    // written.  dec_row [N][C-1][H][tiles_x] and dec_col [N][tiles_y][C-1][W] feed kp_finish (decode.hip); both null = write logits
    float* dec_row;
    float* dec_col;
    int dec_C;                     // real class count incl. background (58)
    int N, H, W;
    int HP, NQ, LC;                // padded hidden width (800), HP/32, padded class count (M2*16)
    int tiles_x, tiles_y;          // filled by the launcher
    unsigned tiles_x_magic, tiles_y_magic;   // filled by the launcher: floor(2^32 / d) + 1
    int stage_folds;               // headx3.hip, filled by the launcher: the folded branches' source boxes of a tile go through LDS once (1) or every lane fetches its taps (0)
    unsigned* range;               // headx3.hip (fp16x3): sticky counter of wavefronts that split a value beyond the fp16 range (x3.hpp), or null
    unsigned long long* trace;     // head32.hip / headx3.hip tuning aid (SNCAL_HEAD_TRACE=<file>): 8 phase sums per workgroup, or null
};

int launch_head_fused(const HeadParams& p, int m2, hipStream_t s);
bool launch_head32(const HeadParams& p, hipStream_t s);      // head32.hip; false = does not apply, nothing launched
bool head32_applies(const HeadParams& p);                  // the same test without launching
size_t head32_decode_scratch(int B, int C, int h, int w);   // bytes of dec_row + dec_col
void head32_decode_parts(int h, int w, int* row_parts, int* col_parts);
// headx3.hip: the same head in split-fp16 arithmetic on fp32 tensors (fp16x3 engine); direct / fold / src are fp32 there
bool launch_headx3(const HeadParams& p, hipStream_t s);
bool headx3_applies(const HeadParams& p);
bool headx3_enabled();                                     // SNCAL_HEADX3 (0 = the split head on the generic fp32 kernels)

// headx4.hip: the fp16x3 head at upscale 4.  No tensor sits at head resolution there, so the stem joins branches 0 and 1 as a third
// blended source of stage 1's K (concat order: stem | branch 0 | branch 1); h.direct is null, h.Cd 0, h.nfold 0 and h.fold unused; h.src
// are the two gathered products as in headx3.
constexpr int HEADX4_FOLD = 3;
struct HeadX4Params {
    HeadParams h;
    const void* fold[HEADX4_FOLD];     // [N][Hf][Wf][Cf] fp32
    int Cf[HEADX4_FOLD], Hf[HEADX4_FOLD], Wf[HEADX4_FOLD];
    float fsy[HEADX4_FOLD], fsx[HEADX4_FOLD];
};
bool launch_headx4(const HeadX4Params& p, hipStream_t s);    // false = does not apply, nothing launched
bool headx4_applies(const HeadX4Params& p);
// the shape half of headx4_applies, for the layout (before the tensors have their shapes): blended sources of fc[] channels at the
// align_corners scales fsy[] / fsx[] towards the head, two gathered products at horizontal scales gsx[]
bool headx4_fits(const int* fc, const float* fsy, const float* fsx, const float* gsx);

// tiles of tile_w x tile_h head pixels and their magic reciprocals (head_tile, head_frame.hpp); returns the block count
inline unsigned head_set_tiling(HeadParams& q, int tile_w, int tile_h) {
    q.tiles_x = (q.W + tile_w - 1) / tile_w;
    q.tiles_y = (q.H + tile_h - 1) / tile_h;
    q.tiles_x_magic = q.tiles_x <= 1 ? 0u : 0xFFFFFFFFu / (unsigned)q.tiles_x + 1u;
    q.tiles_y_magic = q.tiles_y <= 1 ? 0u : 0xFFFFFFFFu / (unsigned)q.tiles_y + 1u;
    return (unsigned)(q.tiles_x * q.tiles_y * q.N);
}
// 32-wide kernels: the worst-case box of a gather source at horizontal scale sx for one output row x 32 columns (2 rows x
// (int)(31 sx) + 3 columns) fits the 16 pixels of one DMA piece / K step
inline bool head_boxes_fit(float sx) { return 2 * ((int)(sx * 31) + 3) <= 16; }

// ---- the packed-weight formats of the fused heads (host; pack.hpp) ------------------------------------------------------------------
// W0 = last_layer.0 (1x1, BN scale folded), W1 = last_layer.3.  Stage 1 multiplies the first K1 concat columns from column coff of W0 on
// (the direct tensor's Cd channels + the folded branches); HP = padded hidden width (NQ = HP / 32 slices), M2 = 16-class fragments.
struct HeadPackShape {
    int HP, M2, Cd, coff, K1, KS1;
    int NQ() const { return HP / 32; }
    int KS16() const { return K1 / 16; }                 // 32x32x16 packing: k-steps of stage 1 (exists when K1 % 16 == 0)
    int RB() const { return (M2 * 16 + 31) / 32; }       // ... 32-row class blocks of stage 2
};
inline bool head_shape_ok(const HeadPackShape& s) { return s.Cd <= 64 && s.M2 <= 4 && s.K1 <= s.KS1 * 32; }      // else no fused head

// head.hip (bf16): the 16x16x32 fragments.  w0 [NQ][2][KS1][64 lanes] x 8 bf16: lane l of fragment f holds hidden channel
// q * 32 + (m >> 2) * 8 + f * 4 + (m & 3), m = l & 15 (row permutation, see head.hip), k = ks * 32 + (l >> 4) * 8 + 0..7 (zeros from K1
// on); w1 [NQ][M2][64 lanes] x 8: class mi * 16 + (l & 15), hidden channel q * 32 + (l >> 4) * 8 + 0..7.
inline size_t head_w0_packed_bytes(const HeadPackShape& s) { return (size_t)s.NQ() * 2 * s.KS1 * 1024; }
inline size_t head_w1_packed_bytes(const HeadPackShape& s) { return (size_t)s.NQ() * s.M2 * 1024; }
inline void head_pack_weights(Folded W0, Folded W1, HeadPackShape s, std::vector<uint16_t>& w0, std::vector<uint16_t>& w1) {
    const int NQ = s.NQ(), KS1 = s.KS1, M2 = s.M2;
    w0.assign(head_w0_packed_bytes(s) / 2, 0);
    w1.assign(head_w1_packed_bytes(s) / 2, 0);
    for (int q = 0; q < NQ; ++q)
        for (int f = 0; f < 2; ++f)
            for (int ks = 0; ks < KS1; ++ks)
                for (int lane = 0; lane < 64; ++lane) {
                    const int m = lane & 15, gk = lane >> 4;
                    const int ch = q * 32 + (m >> 2) * 8 + f * 4 + (m & 3);
                    if (ch >= W0.cout) continue;
                    uint16_t* dst = w0.data() + ((((size_t)(q * 2 + f) * KS1 + ks) * 64) + lane) * 8;
                    for (int e = 0; e < 8; ++e) {
                        const int k = ks * 32 + gk * 8 + e;
                        if (k < s.K1) dst[e] = f2bf(W0.tap<1>(ch, s.coff + k));
                    }
                }
    for (int q = 0; q < NQ; ++q)
        for (int mi = 0; mi < M2; ++mi)
            for (int lane = 0; lane < 64; ++lane) {
                const int cls = mi * 16 + (lane & 15), gk = lane >> 4;
                if (cls >= W1.cout) continue;
                uint16_t* dst = w1.data() + (((size_t)(q * M2 + mi) * 64) + lane) * 8;
                for (int e = 0; e < 8; ++e) {
                    const int k = q * 32 + gk * 8 + e;
                    if (k < W1.cin) dst[e] = f2bf(W1.tap<1>(cls, k));
                }
            }
}

// head32.hip (bf16) / headx3.hip (split engines): the 32x32x16 fragments, K1 a multiple of 16.  w0 [NQ][KS16][64 lanes] x 8: lane l holds
// row h32_row_channel(l & 31) of the 32-row block, k = 16 ks + 8 (l >> 5) + 0..7; w1 [NQ][RB][2][64 lanes] x 8: class rb * 32 + row,
// hidden channel q * 32 + h * 16 + 8 (l >> 5) + 0..7.  split = false: bf16 in w0 / w1, the lo vectors stay empty; split = true: every
// weight as hi + lo (x3.hpp), the lo parts in w0_lo / w1_lo in the same layout.
inline size_t head32_w0_packed_bytes(const HeadPackShape& s) { return (size_t)s.NQ() * s.KS16() * 1024; }
inline size_t head32_w1_packed_bytes(const HeadPackShape& s) { return (size_t)s.NQ() * s.RB() * 2 * 1024; }
inline void head32_pack_weights(Folded W0, Folded W1, HeadPackShape s, bool split, std::vector<uint16_t>& w0,
                                std::vector<uint16_t>& w1, std::vector<uint16_t>& w0_lo, std::vector<uint16_t>& w1_lo) {
    const int NQ = s.NQ(), KS16 = s.KS16(), RB = s.RB();
    w0.assign(head32_w0_packed_bytes(s) / 2, 0);
    w1.assign(head32_w1_packed_bytes(s) / 2, 0);
    w0_lo.assign(split ? w0.size() : 0, 0);
    w1_lo.assign(split ? w1.size() : 0, 0);
    auto put = [&](std::vector<uint16_t>& hi, std::vector<uint16_t>& lo, size_t o, float w) {
        if (split) x3_split_host(w, &hi[o], &lo[o]); else hi[o] = f2bf(w);
    };
    for (int q = 0; q < NQ; ++q)
        for (int lane = 0; lane < 64; ++lane) {
            const int row = h32_row_channel(lane & 31), kb = (lane >> 5) * 8;
            const int ch = q * 32 + row;
            for (int ks = 0; ks < KS16 && ch < W0.cout; ++ks) {
                const size_t o = (((size_t)q * KS16 + ks) * 64 + lane) * 8;
                for (int e = 0; e < 8; ++e) put(w0, w0_lo, o + e, W0.tap<1>(ch, s.coff + ks * 16 + kb + e));
            }
            for (int rb = 0; rb < RB; ++rb)
                for (int h = 0; h < 2; ++h) {
                    const int cls = rb * 32 + row;
                    if (cls >= W1.cout) continue;
                    const size_t o = ((((size_t)q * RB + rb) * 2 + h) * 64 + lane) * 8;
                    for (int e = 0; e < 8; ++e) {
                        const int k = q * 32 + h * 16 + kb + e;
                        if (k < W1.cin) put(w1, w1_lo, o + e, W1.tap<1>(cls, k));
                    }
                }
        }
}

// the two bias vectors of every form: b0 [HP] folded-BN shift of last_layer.0, b1 the bias of last_layer.3 -- at least 64 slots: head32's
// decode epilogue reads 64 whatever the class count
inline void head_pack_bias(const float* shift0, int cout0, const float* shift1, int cout1, HeadPackShape s, std::vector<float>& b0,
                           std::vector<float>& b1) {
    b0.assign(s.HP, 0.f);
    b1.assign((size_t)std::max(s.M2 * 16, 64), 0.f);
    for (int co = 0; co < cout0; ++co) b0[co] = shift0[co];
    for (int c = 0; c < cout1; ++c) b1[c] = shift1[c];
}

}  // namespace sncal
