// Two-team persistent 3x3 convolution (conv_tt.hip): tile geometry, parameters, work items and their plan, launcher, weight packing.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>
#include "pack.hpp"
#include "x3.hpp"        // x3_split_host

namespace sncal {

constexpr int TT_MAX_MEMBERS = 3;
constexpr int TT_CIN = 32;          // input channels per stage (G = 4 k-groups of 8 bf16)
constexpr int TT_TABLE_MAX = 760;       // floats per LDS table (bias, output scale)
constexpr int TT_QUEUE_FLOATS = 16;     // the LAST 16 floats of the output-scale table are the ticket queue's four TTItem slots (conv_tt_kernel.hpp q_slot)
constexpr int TT_COUT_MAX = TT_TABLE_MAX - TT_QUEUE_FLOATS;      // so a (grouped) launch may hold at most this many output channels in its tables

// The geometry of one tile shape, stated here for the kernel (conv_tt_kernel.hpp) and the host alike.
// tile of an instantiation: MB 32-channel blocks x (4 NB) stacked rows x 32 columns per team; a wave owns NB rows
template <int MB_, int NB_>
struct TTShape {
    static constexpr int MB = MB_, NB = NB_, NT = 18;           // 32-channel blocks, 32-pixel blocks (= tile rows) per wave, K = 16 steps per stage
    static constexpr int COUT_BLK = 32 * MB;                    // output channels per work item (MI fragments)
    static constexpr int TILE_H = 4 * NB;                       // output rows per tile (rows of the STACKED image, see conv_tt.hip)
    static constexpr int TILE_W = 32;                           // output columns per tile (two 16-pixel MFMA fragments)
    static constexpr int NKS = 9, MI = 2 * MB;                  // taps; 1 KB weight pieces per tap
    static constexpr int W_BYTES = NKS * MI * 1024;             // one stage of weights, fragment order [k-step][mi][lane] x 16 B
    static constexpr int HP = 36;                               // halo row pitch in pixels (34 used)
    static constexpr int HROWS = TILE_H + 2;
    static constexpr int HALO_PIECES = (HROWS * HP * 64 + 1023) / 1024;     // DMA pieces of 1 KB
    static constexpr int HV = (HALO_PIECES + 3) / 4;            // ... per wave
    static constexpr int H_BYTES = HALO_PIECES * 1024;
    static constexpr int TEAM_BYTES = W_BYTES + H_BYTES;        // (3, 2): 78848, two teams = 157696 B of the CU's 163840; (2, 3): 69632
    static constexpr int LDS_BYTES = 2 * TEAM_BYTES + 64 + 2 * TT_TABLE_MAX * 4;     // dynamic LDS of a launch: two teams, the hand-shake words, the two tables
    // weight pieces per wave: wave tw owns a CONTIGUOUS block [wp_first(tw), wp_first(tw + 1)), because the wave also stages its epilogue there
    static __device__ __host__ constexpr int wp_first(int tw) { return tw * (NKS * MI) / 4; }
    static constexpr int EPI_PITCH = COUT_BLK + 4;              // floats per staged pixel row
    static constexpr int EPI_GROUPS = COUT_BLK / 8, EPI_ITEMS = 32 * EPI_GROUPS, EPI_ITERS = EPI_ITEMS / 64;
    static_assert(32 * EPI_PITCH * 4 <= (NKS * MI / 4) * 1024 && EPI_ITEMS % 64 == 0 && LDS_BYTES <= 160 * 1024,
                  "a wave's epilogue staging must fit its own block of the weight region; two teams fit the CU's LDS");
    static constexpr bool blocks_cover() { return wp_first(4) == NKS * MI; }        // (asserted below: not callable before the class is complete)
};
static_assert(TTShape<3, 2>::blocks_cover() && TTShape<2, 3>::blocks_cover() && TTShape<3, 1>::blocks_cover(), "the four waves' blocks are the whole weight region");

// ---- the tile shapes: (MB, NB) = (3, 2): 96 output channels x 8 stacked rows x 32 columns, every mode;
//      (2, 3): 64 x 12 x 32 for the bf16x3 engine's 48-channel branch (25 % instead of 50 % of padded rows);
//      (3, 1): 96 x 4 x 32, split arithmetic only -- SMALL launches (conv_tt.hip)
enum TTTile { TT_TILE_96x8 = 0, TT_TILE_64x12 = 1, TT_TILE_96x4 = 2 };
using TTShape96x8 = TTShape<3, 2>;
using TTShape64x12 = TTShape<2, 3>;
using TTShape96x4 = TTShape<3, 1>;
struct TTTileInfo { int cout_blk, tile_h, tile_w, lds_bytes; const char* label; };     // label: the tile as the profile rows name it
template <class S> constexpr TTTileInfo tt_tile_info(const char* label) { return {S::COUT_BLK, S::TILE_H, S::TILE_W, S::LDS_BYTES, label}; }
constexpr TTTileInfo TT_TILES[3] = {tt_tile_info<TTShape96x8>("8x32x96"), tt_tile_info<TTShape64x12>("12x32x64"), tt_tile_info<TTShape96x4>("4x32x96")};
constexpr int TT_COUT = TTShape96x8::COUT_BLK;      // channel block of the bf16 and fp8 layers, and of the split engine's layers where it divides the width

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
    // fp8 variant only (MODE 1): y = acc * oscale[c] + bias[c] with oscale = input scale x weight scale of channel c
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
    int lazy;                       // 1: small launch -- a workgroup draws its next ticket only when its pair is done (conv_tt_kernel.hpp)
    unsigned long long* trace;      // tuning aid (SNCAL_TT_TRACE=<file>): 256 s_memtime stamps per team, or null
    int ablate;                     // tuning aid (SNCAL_TT_ABLATE, timing only, results invalid): 1 = no epilogue, 2 = no MFMAs, 4 = no DMA
};

// mode 0 bf16, 1 fp8 (e4m3), 2 x3 (split-bf16, fp32 in / out); every mode runs on TT_TILE_96x8, mode 2 also on the other two tiles.
// SNCAL_ERR_ARG for a (tile, mode) pair that has no kernel.
int launch_conv_tt(const TTParams& p, int n_wgs, int mode, hipStream_t s, TTTile tile = TT_TILE_96x8);

// ---- the work items of a launch (host, no device involved: tools/dev/tt_plan_host_check.cpp runs it stand-alone) ----
struct TTGrid {                     // the items of one member: tiles_y x tiles_x tiles, tile-major, the nblk channel blocks of a tile adjacent
    int tiles_y, tiles_x, nblk;
    long items() const { return (long)tiles_y * tiles_x * nblk; }
};
inline TTGrid tt_grid(int N, int H, int W, int cout, TTTile tile) {
    const TTTileInfo& t = TT_TILES[tile];
    return {(N * (H + 1) + t.tile_h - 1) / t.tile_h, (W + t.tile_w - 1) / t.tile_w, (cout + t.cout_blk - 1) / t.cout_blk};
}

struct TTPlan { std::vector<TTItem> items; uint32_t first[9]; int lazy; };
// The work items of the member convolutions as eight queues, one per XCD.  Workgroup b runs on XCD b % 8 (observed
// dispatch rule, used for speed only): every member's items -- tile-major, the 96-channel blocks of a tile adjacent --
// are cut into 8 contiguous slices, one per XCD, so that neighbouring tiles (shared halo rows) and the blocks of one
// tile (same input) meet in one L2; inside an XCD's queue the members follow each other, most expensive first
// (longest-processing-time order: the teams, which take the next item when they finish one, end within one cheap item
// of each other).  Rounds 2-4 dealt the items to the teams HERE (static lists); a workgroup whose CU was held by a
// camera-solve wavefront then started when the first other workgroup had finished, and the launch lasted twice as long.
inline TTPlan tt_plan_items(const TTMember* mem, int n, TTTile tile, int n_wgs) {
    const TTTileInfo& t = TT_TILES[tile];
    const int n_xcd = n_wgs >= 8 ? 8 : 1;                  // (fewer than 8 workgroups: every workgroup reads queue b % 8, so only queue 0.. exist)
    std::vector<std::vector<TTItem>> per_xcd(8);
    int order[TT_MAX_MEMBERS] = {0, 1, 2};
    std::sort(order, order + n, [&](int a, int b) { return mem[a].chunks > mem[b].chunks; });
    // (Interleaving the members' items, so that the memory-heavy 96-channel tiles do not all run at the tail of the launch, measured
    // 1.4 % SLOWER than member after member: 193.3 vs 190.6 us per grouped launch; the two teams of a workgroup walking the classes in
    // OPPOSITE order measured 1.7 % slower on the fp16x3 launches, round 4.)
    for (int oi = 0; oi < n; ++oi) {
        const TTMember& m = mem[order[oi]];
        const TTGrid g = tt_grid(m.N, m.H, m.W, m.cout, tile);
        const long total = g.items();
        for (long i = 0; i < total; ++i) {
            const int x = n_xcd == 8 ? (int)(i * 8 / total) : 0;
            TTItem it;
            it.member = (uint16_t)order[oi]; it.nb = (uint16_t)(i % g.nblk);
            const long tl = i / g.nblk;
            it.col0 = (int32_t)(tl % g.tiles_x) * t.tile_w; it.row0 = (int32_t)(tl / g.tiles_x) * t.tile_h; it.pad_ = 0;
            per_xcd[x].push_back(it);
        }
    }
    // (Measured and not kept, round 5: the tickets of a member's slice S-way interleaved -- S = 4, 8, 16, 64 -- so that the items that share
    // halo lines are not drawn at the same instant: 32.87 / 33.06 / 32.95 / 33.10 ms per step of two-team launches against 32.85 in
    // tile-major order, FETCH_SIZE 434 against 410 MB per launch.  The queue's extra HBM reads over round 4's static deal -- 412 against
    // 310 MB per grouped launch by PMC -- are not concurrent misses of neighbouring tickets.)
    TTPlan plan;
    for (int x = 0; x < 8; ++x) { plan.first[x] = (uint32_t)plan.items.size(); plan.items.insert(plan.items.end(), per_xcd[x].begin(), per_xcd[x].end()); }
    plan.first[8] = (uint32_t)plan.items.size();
    if (plan.items.empty()) plan.items.push_back(TTItem{0, 0, 0, 0, 0});
    // fewer than 8 pairs of items per workgroup in an XCD's list: the kernel's three-pairs-ahead ticket pipeline would starve most workgroups
    plan.lazy = plan.items.size() < (size_t)3 * (size_t)n_wgs ? 1 : 0;      // fewer than 1.5 pairs per workgroup
    return plan;
}

// ---- the three packed-weight formats of the kernel (host; pack.hpp): one stage of A fragments per (output-channel block nb, input-
// channel chunk c), a layer = [nb][c] stages.  W: the folded 3x3 weights of the layer.
// bf16 (mode 0): wide 3x3 stride-1 layers.  Stage [tap 9][channel half 2][32-row block 3][lane 64] x 8 bf16 = 54 KB, the A fragments of
// v_mfma_f32_32x32x16_bf16: lane l holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 32 + h * 16 + (l >> 5) * 8 + 0..7.
inline bool tt_shape_ok(int k, int stride, int cin, int cin_phys, int cout) {
    return k == 3 && stride == 1 && cin == cin_phys && cin % TT_CIN == 0 && cout % TT_COUT == 0 && cout <= 480;
}
inline int tt_chunks(int cin) { return cin / TT_CIN; }
inline size_t tt_packed_bytes(int cin, int cout) { return (size_t)(cout / TT_COUT) * tt_chunks(cin) * TTShape96x8::W_BYTES; }
inline void tt_pack_weights(Folded W, std::vector<uint16_t>& out) {
    using S = TTShape96x8;
    const int chunks = tt_chunks(W.cin), nblk = W.cout / TT_COUT;
    out.assign(tt_packed_bytes(W.cin, W.cout) / 2, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < S::NKS; ++s)
                for (int h = 0; h < 2; ++h)
                    for (int mb = 0; mb < S::MB; ++mb)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint16_t* dst = out.data() + ((((((size_t)nb * chunks + c) * S::NKS + s) * 2 + h) * S::MB + mb) * 64 + lane) * 8;
                            for (int e = 0; e < 8; ++e) dst[e] = f2bf(W.tap<3>(co, c * TT_CIN + h * 16 + (lane >> 5) * 8 + e, s));
                        }
}

// e4m3 (mode 1), the same layers: 64-channel chunks, stage [tap 9][32-row block 3][half 2][lane 64] x 16 e4m3 = 54 KB, the A operand of
// v_mfma_scale_f32_32x32x64_f8f6f4: lane l holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 64 + 32 (l >> 5) +
// 16 half + 0..15 of the tap (zeros beyond Cin).  One scale per output channel: wscale = max |w| / 448 over the channel's folded weights.
inline int tt8_chunks(int cin) { return (cin + 63) / 64; }
inline size_t tt8_packed_bytes(int cin, int cout) { return (size_t)(cout / TT_COUT) * tt8_chunks(cin) * TTShape96x8::W_BYTES; }
inline void tt8_pack_weights(Folded W, std::vector<uint8_t>& out, std::vector<float>& wscale) {
    using S = TTShape96x8;
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
            for (int s = 0; s < S::NKS; ++s)
                for (int mb = 0; mb < S::MB; ++mb)
                    for (int half = 0; half < 2; ++half)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint8_t* dst = base + (((((((size_t)nb * chunks + c) * S::NKS + s) * S::MB + mb) * 2 + half) * 64) + lane) * 16;
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
// (conv_tt_kernel.hpp x3_quad_channel); hi = rne16(w), lo = rne16(w - hi) (x3.hpp).
inline bool x3_shape_ok(int k, int stride, int stage, int cin, int cin_phys, int cout) {
    return k == 3 && stride == 1 && stage >= 2 && cin == cin_phys && cin % 16 == 0 && cout % 16 == 0 && cout <= 480;
}
inline int ttx3_block(int cout) { return cout % TT_COUT == 0 ? TT_COUT : TTShape64x12::COUT_BLK; }
inline int ttx3_chunks(int cin) { return cin / 16; }
constexpr size_t ttx3_stage_bytes(int blk) { return (size_t)TTShape96x8::NKS * 2 * (blk / 32) * 1024; }       // W_BYTES of the tile whose channel block is blk
static_assert(ttx3_stage_bytes(TTShape96x8::COUT_BLK) == TTShape96x8::W_BYTES && ttx3_stage_bytes(TTShape64x12::COUT_BLK) == TTShape64x12::W_BYTES, "");
inline size_t ttx3_packed_bytes(int cin, int cout, int blk) { return (size_t)((cout + blk - 1) / blk) * ttx3_chunks(cin) * ttx3_stage_bytes(blk); }
inline void ttx3_pack_weights(Folded W, int blk, std::vector<uint16_t>& out) {
    constexpr int NKS = TTShape96x8::NKS;
    const int MBk = blk / 32, chunks = ttx3_chunks(W.cin), nblk = (W.cout + blk - 1) / blk;
    out.assign(ttx3_packed_bytes(W.cin, W.cout, blk) / 2, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < NKS; ++s)
                for (int mb = 0; mb < MBk; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int co = nb * blk + mb * 32 + h32_row_channel(lane & 31);
                        if (co >= W.cout) continue;
                        uint16_t* hi = out.data() + ((((((size_t)nb * chunks + c) * NKS + s) * 2 + 0) * MBk + mb) * 64 + lane) * 8;
                        uint16_t* lo = out.data() + ((((((size_t)nb * chunks + c) * NKS + s) * 2 + 1) * MBk + mb) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) x3_split_host(W.tap<3>(co, c * 16 + (lane >> 5) * 8 + e, s), &hi[e], &lo[e]);
                    }
}

}  // namespace sncal
