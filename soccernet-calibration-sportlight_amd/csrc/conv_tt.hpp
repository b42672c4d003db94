// Two-team persistent 3x3 convolution (conv_tt.hip): parameters, work items, launcher, weight packing.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>
#include "pack.hpp"
#include "x3.hpp"        // x3_split_host

namespace sncal {

constexpr int TT_MAX_MEMBERS = 3;
constexpr int TT_TH = 8;            // output rows per tile (rows of the STACKED image, see conv_tt.hip)
constexpr int TT_TW = 32;           // output columns per tile (two 16-pixel MFMA fragments)
constexpr int TT_COUT = 96;         // output channels per work item (MI = 6 fragments)
constexpr int TT_CIN = 32;          // input channels per stage (G = 4 k-groups of 8 bf16)

struct TTMember {                   // one convolution of the launch: 3x3, stride 1, pad 1, bf16 NHWC, folded BN (+res)(+ReLU)
    const void* in;                 // [N][H][W][Cin] bf16 (fp8 variant: the e4m3 twin of the tensor, 1 byte per element)
    void* out;                      // [N][H][W][out_cstride] bf16, channels at out_coff (fp8 variant: may be NULL)
    const void* res;                // optional residual, indexed like out
    const void* w;                  // packed weights of the mode: tt_pack_weights / tt8_pack_weights / ttx3_pack_weights (below)
    const float* bias;              // folded-BN shift, padded to nblk * 96
    int N, H, W, Cin, chunks;       // chunks = Cin / 32
    int cout, out_cstride, out_coff, relu;
    unsigned w_bytes, in_bytes;     // buffer-descriptor ranges
    unsigned hp1_magic;             // floor(2^32 / (H + 1)) + 1
    // fp8 variant only (conv_tt_kernel<true>): y = acc * oscale[c] + bias[c] with oscale = input scale x weight scale of channel c
    const float* oscale;            // [cout]
    void* out8;                     // optional e4m3 twin of the output, indexed like out at 1 byte per element
    float out8_inv_scale;           // 1 / (per-tensor scale of the output twin)
    int res_split;                  // bf16x3: res points at the residual's SPLIT TWIN ([16 hi | 16 lo] bf16 per 16-channel group, dense), not at fp32
};

struct TTItem {                     // one output tile x one 96-channel block
    uint16_t member, nb;
    int32_t row0;                   // first STACKED output row of the tile (frame f, row y  ->  f * (H + 1) + y)
    int32_t col0;
    int32_t pad_;
};

struct TTParams {
    TTMember m[TT_MAX_MEMBERS];
    const TTItem* items;            // grouped by XCD (workgroup b runs on XCD b % 8), most expensive member first inside an XCD
    const uint32_t* xcd_first;      // [9] offsets into items
    unsigned* queue;                // sixteen zeroed device words owned by the caller's stream: next item per XCD [0..8), teams that have left per XCD [8..16)
                                    // (the kernel re-arms them; launches that share the words must be ordered on one stream)
    unsigned* range;                // fp16x3: sticky counter of wavefronts that split a value beyond the fp16 range (x3.hpp x3_report), or null
    int lazy;                       // 1: small launch -- a workgroup draws its next ticket only when its pair is done (conv_tt_body.inc)
    unsigned long long* trace;      // tuning aid (SNCAL_TT_TRACE=<file>): 256 s_memtime stamps per team, or null
    int ablate;                     // tuning aid (SNCAL_TT_ABLATE, timing only, results invalid): 1 = no epilogue, 2 = no MFMAs, 4 = no DMA
};

void launch_conv_tt(const TTParams& p, int n_wgs, int mode, hipStream_t s, int cfg = 0);      // mode 0 bf16, 1 fp8 (e4m3), 2 x3 (split-bf16, fp32 in / out);
                                                                                                // cfg 0: 96 channels x 8 rows, 1: 64 x 12 (mode 2 only)
constexpr int TT_TABLE_MAX = 760;       // floats per LDS table (bias, output scale)
constexpr int TT_QUEUE_FLOATS = 16;     // the LAST 16 floats of the output-scale table are the ticket queue's four TTItem slots (conv_tt_body.inc q_slot)
constexpr int TT_COUT_MAX = TT_TABLE_MAX - TT_QUEUE_FLOATS;      // so a (grouped) launch may hold at most this many output channels in its tables

// ---- the three packed-weight formats of the kernel (host; pack.hpp): one stage of A fragments per (output-channel block nb, input-
// channel chunk c), a layer = [nb][c] stages.  W: the folded 3x3 weights of the layer.
// bf16 (mode 0): wide 3x3 stride-1 layers.  Stage [tap 9][channel half 2][32-row block 3][lane 64] x 8 bf16 = 54 KB, the A fragments of
// v_mfma_f32_32x32x16_bf16: lane l holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 32 + h * 16 + (l >> 5) * 8 + 0..7.
inline bool tt_shape_ok(int k, int stride, int cin, int cin_phys, int cout) {
    return k == 3 && stride == 1 && cin == cin_phys && cin % TT_CIN == 0 && cout % TT_COUT == 0 && cout <= 480;
}
inline int tt_chunks(int cin) { return cin / TT_CIN; }
inline size_t tt_packed_bytes(int cin, int cout) { return (size_t)(cout / TT_COUT) * tt_chunks(cin) * 9 * 2 * 3 * 1024; }
inline void tt_pack_weights(Folded W, std::vector<uint16_t>& out) {
    const int chunks = tt_chunks(W.cin), nblk = W.cout / TT_COUT;
    out.assign(tt_packed_bytes(W.cin, W.cout) / 2, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int h = 0; h < 2; ++h)
                    for (int mb = 0; mb < 3; ++mb)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint16_t* dst = out.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + h) * 3 + mb) * 64 + lane) * 8;
                            for (int e = 0; e < 8; ++e) dst[e] = f2bf(W.tap<3>(co, c * TT_CIN + h * 16 + (lane >> 5) * 8 + e, s));
                        }
}

// e4m3 (mode 1), the same layers: 64-channel chunks, stage [tap 9][32-row block 3][half 2][lane 64] x 16 e4m3 = 54 KB, the A operand of
// v_mfma_scale_f32_32x32x64_f8f6f4: lane l holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 64 + 32 (l >> 5) +
// 16 half + 0..15 of the tap (zeros beyond Cin).  One scale per output channel: wscale = max |w| / 448 over the channel's folded weights.
inline int tt8_chunks(int cin) { return (cin + 63) / 64; }
inline size_t tt8_packed_bytes(int cin, int cout) { return (size_t)(cout / TT_COUT) * tt8_chunks(cin) * 9 * 3 * 2 * 1024; }
inline void tt8_pack_weights(Folded W, std::vector<uint8_t>& out, std::vector<float>& wscale) {
    const int chunks = tt8_chunks(W.cin), nblk = W.cout / TT_COUT;
    wscale.assign(W.cout, 1.f);
    for (int co = 0; co < W.cout; ++co) {
        const float mx = W.max_abs(co);
        wscale[co] = mx > 0.f ? mx / 448.f : 1.f;
    }
    out.assign(tt8_packed_bytes(W.cin, W.cout), 0);
    uint8_t* const base = out.data();
    const float* const ws = wscale.data();
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int mb = 0; mb < 3; ++mb)
                    for (int half = 0; half < 2; ++half)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint8_t* dst = base + (((((((size_t)nb * chunks + c) * 9 + s) * 3 + mb) * 2 + half) * 64) + lane) * 16;
                            for (int e = 0; e < 16; ++e) {
                                const int ci = c * 64 + 32 * (lane >> 5) + 16 * half + e;
                                if (ci < W.cin) dst[e] = f2fp8(W.tap<3>(co, ci, s) / ws[co]);
                            }
                        }
}

// split engine (mode 2), 3x3 stride-1 layers of stages 2-4 from 16 channels on: 16-channel chunks, stage [tap 9][part: hi, lo][32-row
// block MB][lane 64] x 8 codes -- the bf16 stage layout with its two K = 16 steps holding the hi and the lo parts of the SAME 16 input
// channels, in output-channel blocks of blk = 96 or, for widths that are no multiple of 96, 64 (48 channels: 25 % zero rows instead of
// 50 %).  Lane l holds output channel nb * blk + mb * 32 + h32_row_channel(l & 31) (zero rows above the layer's width), input channels
// c * 16 + (l >> 5) * 8 + 0..7 of the tap: a lane's accumulator registers 8 p .. 8 p + 7 are then 8 consecutive channels
// (conv_tt_body.inc x3_quad_channel); hi = rne16(w), lo = rne16(w - hi) (x3.hpp).
inline bool x3_shape_ok(int k, int stride, int stage, int cin, int cin_phys, int cout) {
    return k == 3 && stride == 1 && stage >= 2 && cin == cin_phys && cin % 16 == 0 && cout % 16 == 0 && cout <= 480;
}
inline int ttx3_block(int cout) { return cout % TT_COUT == 0 ? TT_COUT : 64; }
inline int ttx3_chunks(int cin) { return cin / 16; }
inline size_t ttx3_packed_bytes(int cin, int cout, int blk) { return (size_t)((cout + blk - 1) / blk) * ttx3_chunks(cin) * 9 * 2 * (blk / 32) * 1024; }
inline void ttx3_pack_weights(Folded W, int blk, std::vector<uint16_t>& out) {
    const int MBk = blk / 32, chunks = ttx3_chunks(W.cin), nblk = (W.cout + blk - 1) / blk;
    out.assign(ttx3_packed_bytes(W.cin, W.cout, blk) / 2, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int mb = 0; mb < MBk; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int co = nb * blk + mb * 32 + h32_row_channel(lane & 31);
                        if (co >= W.cout) continue;
                        uint16_t* hi = out.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + 0) * MBk + mb) * 64 + lane) * 8;
                        uint16_t* lo = out.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + 1) * MBk + mb) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) x3_split_host(W.tap<3>(co, c * 16 + (lane >> 5) * 8 + e, s), &hi[e], &lo[e]);
                    }
}

}  // namespace sncal
