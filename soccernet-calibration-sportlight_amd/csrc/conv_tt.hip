// Two-team persistent 3x3 stride-1 convolution for the wide HRNet branches (96 / 192 / 384 channels), bf16.
//
// Replaces, for these layers, the conv3x3 + eval-BN (+ residual) (+ ReLU) of BasicBlock
// (/root/reference/src/models/hrnet/hrnet.py:42-58) that the generic kernel (conv.hpp) runs as
// conv<bf16,k3,s1,NI3,MI6,G4>.  Same GEMM view (D[cout, pixel] = sum_k W[cout, k] X[k, pixel], k = chunk of 32 input
// channels -> tap -> channel), same bf16 operands, fp32 accumulation started at the folded-BN shift, same epilogue
// arithmetic.  The MFMA shape is v_mfma_f32_32x32x16_bf16 (the generic kernel: 16x16x32): the products of one output are
// summed in a different order inside the matrix unit, so outputs agree with the generic kernel to fp32 rounding of the
// accumulator, not bit for bit (the first version of this kernel used 16x16x32 and WAS bit-identical; a phase trace
// showed 216 of them take 4.1k clk per wave where 108 of the 32x32x16 take 3.5k -- MI355X_MICROARCH.md: 2075 vs 2382 TF).
//
// Why another kernel.  The generic kernel stages a chunk (54 KB of weights + the halo tile), waits, multiplies, and
// relies on a second resident workgroup to fill the wait.  Measured (NOTES/design_history_r1_r5.md §4): the two workgroups drift into
// phase, the LDS-DMA issue of one (~100 clk per 1 KB piece on the issuing wave) lands on top of its own MFMA phase
// as often as under the other's, and the MFMA pipe is busy 40 % of the kernel although the work is MFMA-bound.
// Here the alternation is BUILT IN:
//   * one workgroup of 8 waves per CU = two TEAMS of 4 waves; wave i of team A and wave i of team B share SIMD i;
//   * one team MULTIPLIES the stage it has in LDS (9 k-steps x 24 MFMAs per wave, one wave per SIMD issuing back to
//     back) while the other team LOADS its next stage by LDS-DMA (its waves carry the whole issue cost and the wait);
//     a token in LDS makes the two MFMA phases mutually exclusive, so the roles swap by themselves (see the main loop);
//   * a team's tile is 8 x 32 output pixels x 96 output channels (4 x 6 accumulator fragments per wave), a stage is
//     32 input channels: 54 KB of weights + a 10 x 34 pixel halo (22.5 KB); two teams = 160 KB of LDS, all of it;
//   * the epilogue of a finished tile runs at the head of the team's next LOAD phase; each wave transposes its fragments
//     through the block of the weight region that it alone refills afterwards, so no team-level barrier is needed;
//   * weights per MAC drop by a quarter against the 192-pixel tile of the generic kernel, and no DMA instruction is
//     ever issued by a wave that has MFMAs to issue.
// Frames are STACKED: output row index s = f * (H + 1) + y, every frame followed by one shared all-zero row (it is the
// bottom padding of frame f and the top padding of frame f + 1).  Tiles of 8 stacked rows then cut the whole batch with
// 1 / (H + 1) waste instead of (ceil(H / 8) * 8 - H) / H per frame -- 6 % instead of 41 % on the 17 x 30 branch.
// The halo image in LDS is [pixel][4 x 16 B] at a 36-pixel row pitch with the four 8-channel groups of a pixel rotated
// by (pixel >> 2) & 3: every ds_read_b128 lane group of a B fragment (32 consecutive pixels, one channel group per
// half-wave) then touches 16 distinct 16-byte bank slots (enumerated against MI355X_MICROARCH.md "LDS"), without the 50 % pitch padding of the generic kernel; the
// rotation is applied on the DMA's per-lane SOURCE address, the LDS destination stays lane-linear.
// Work items (tile x 96-channel block, cost = Cin / 32 stages) of up to three member convolutions are dealt to the
// 2 x 256 teams on the host (tt_plan_items, conv_tt.hpp): contiguous slices per XCD, longest-processing-time first.
#include "conv_tt_kernel.hpp"

namespace sncal {

// ---- the instantiated (tile, mode) pairs.  TT_TILE_96x8 runs every mode; TT_TILE_64x12 is the bf16x3 engine's 48-channel branch (25 %
//      instead of 50 % of padded rows).
// TT_TILE_96x4, split arithmetic only -- SMALL launches (round 5).  Below about two items per team the launch lasts as long as its
// longest item (twelve stages on the 384-channel branch) while most teams hold three-stage items or nothing: at batch 8, 98 us per
// grouped launch for 40 us of work per team.  Half the rows per item = twice the items at half a stage's multiplies each; the weight
// stream per stage is the same (L2 serves it; at these sizes nothing is bandwidth-bound).
struct TTKernel { TTTile tile; int mode; void (*kernel)(const TTParams); };
static const TTKernel tt_kernels[] = {
    {TT_TILE_96x8, 0, conv_tt_kernel<3, 2, 0>}, {TT_TILE_96x8, 1, conv_tt_kernel<3, 2, 1>}, {TT_TILE_96x8, 2, conv_tt_kernel<3, 2, 2>},
    {TT_TILE_64x12, 2, conv_tt_kernel<2, 3, 2>}, {TT_TILE_96x4, 2, conv_tt_kernel<3, 1, 2>},
};

int launch_conv_tt(const TTParams& p, int n_wgs, int mode, hipStream_t s, TTTile tile) {
    if (!opt_in_lds<&conv_tt_kernel<3, 2, 0>, &conv_tt_kernel<3, 2, 1>, &conv_tt_kernel<3, 2, 2>, &conv_tt_kernel<2, 3, 2>, &conv_tt_kernel<3, 1, 2>>(160 * 1024))
        return SNCAL_ERR_HIP;
    for (const TTKernel& k : tt_kernels)
        if (k.tile == tile && k.mode == mode) {
            SNCAL_LAUNCH(k.kernel, dim3((unsigned)n_wgs), dim3(512), (size_t)TT_TILES[tile].lds_bytes, s, p);
            return SNCAL_OK;
        }
    set_error("conv_tt: no kernel for tile %d in mode %d", (int)tile, mode);
    return SNCAL_ERR_ARG;
}

}  // namespace sncal
