// The two-team kernel (conv_tt.hip has the design): one template over the tile shape (MB, NB -- TTShape<MB, NB>, conv_tt.hpp, owns the
// geometry) and the arithmetic mode.
#pragma once
#include "persist.hpp"
#include "conv_tt.hpp"
#include "x3.hpp"
#include <cstddef>

namespace sncal {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((address_space(3))) void lds_void;

// member m's parameters straight from the kernel-argument segment, by scalar loads at a computed offset (selecting among three
// by-value copies of the argument keeps ~80 SGPRs alive and spills; a dynamically indexed argument is copied to scratch)
__device__ __forceinline__ TTMember load_member(int m) {
    TTMember r;
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(TTMember) % 4 == 0 && offsetof(TTParams, m) == 0, "the members must open the kernel-argument segment");
    const __attribute__((address_space(4))) unsigned* src =
        (const __attribute__((address_space(4))) unsigned*)__builtin_amdgcn_kernarg_segment_ptr() + m * (int)(sizeof(TTMember) / 4);
    unsigned* dst = reinterpret_cast<unsigned*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(TTMember) / 4; ++i) dst[i] = src[i];
#else
    (void)m;
    r = TTMember{};
#endif
    return r;
}

// bf16x3: channel (inside its 32-channel block) of the first of the 4 accumulator registers of quad q in lane half hi.  The natural MFMA
// order is 8 q + 4 hi; the x3 weights are packed with rows permuted (ttx3_pack_weights, conv_tt.hpp) so that it is 16 (q / 2) + 8 hi +
// 4 (q % 2): registers 8 p .. 8 p + 7 of a lane are then channels 16 p + 8 hi + 0..7 -- one 16-byte half of a split-twin group.
__device__ __host__ constexpr int x3_quad_channel(int q, int hi) { return 16 * (q >> 1) + 8 * hi + 4 * (q & 1); }
static_assert([] {
    for (int q = 0; q < 4; ++q)
        for (int hi = 0; hi < 2; ++hi)
            for (int j = 0; j < 4; ++j)
                if (h32_row_channel(8 * q + 4 * hi + j) != x3_quad_channel(q, hi) + j) return false;
    return true;
}(), "the epilogue's channel of an accumulator register is the packer's channel of that MFMA row (h32_row_channel, pack.hpp)");

// The MULTIPLY phase of one stage: the wave's MB x NB accumulators += the stage in LDS.  aptr: this lane's 16 bytes of the first weight
// piece; bptr[dx][k]: the lane-dependent part of its B fragment addresses (the kernel has the layout); near_end() runs shortly before the
// last MFMAs are issued (the team hands the CU's multiply token on there).
template <int MB, int NB, int MODE, class F>
__device__ __forceinline__ void tt_multiply_stage(f32x16 (&acc)[MB][NB], const char* const aptr, const char* (&bptr)[3][4], F&& near_end) {
    using S = TTShape<MB, NB>;
    constexpr bool FP8 = MODE == 1, X3 = MODE == 2;
    constexpr int NKS = S::NKS, NT = S::NT, HP = S::HP;
    // pin the accumulators where they are: without this hipcc copies the 96 registers on entry (two reaching
    // definitions: the start value of a new item / the previous stage) and spills some of the originals around the phase
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int jr = 0; jr < NB; ++jr) asm volatile("" : "+v"(acc[mb][jr]));
    if constexpr (FP8) {
        // fp8 stage = 64 input channels: 9 K = 64 steps (one per tap) x 6 v_mfma_scale_f32_32x32x64_f8f6f4 with unit block
        // scales (E8M0 127).  Lane l holds 32 consecutive K bytes of row / column l & 31: channels 32 (l >> 5) .. + 31 of
        // the tap = two 16-byte slots of the pixel, two lane-linear 1 KB pieces of the weights (layout probed on hardware:
        // tools/dev/mx_probe.hip).
        i32x8 a[2][MB], b[2][NB];
        auto load_frags = [&](int s, int buf) {
            const int dy = s / 3, dx = s - dy * 3;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const i32x4 lo = *reinterpret_cast<const i32x4*>(aptr + ((s * MB + mb) * 2 + 0) * 1024);
                const i32x4 hi4 = *reinterpret_cast<const i32x4*>(aptr + ((s * MB + mb) * 2 + 1) * 1024);
                a[buf][mb] = i32x8{lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]};
            }
#pragma unroll
            for (int jr = 0; jr < NB; ++jr) {
                const i32x4 lo = *reinterpret_cast<const i32x4*>(bptr[dx][(jr + dy) & 3] + (jr + dy) * HP * 64);
                const i32x4 hi4 = *reinterpret_cast<const i32x4*>(bptr[dx][(jr + dy + 1) & 3] + (jr + dy) * HP * 64);
                b[buf][jr] = i32x8{lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]};
            }
        };
        load_frags(0, 0);
#pragma unroll
        for (int t = 0; t < NKS; ++t) {
            const int cur = t & 1;
            if (t + 1 < NKS) {
                load_frags(t + 1, cur ^ 1);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int jr = 0; jr < NB; ++jr)
                    acc[mb][jr] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[cur][mb], b[cur][jr], acc[mb][jr], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
            // anchor the step: hipcc sinks the scaled MFMAs of ALL steps below the last reads otherwise (sched_barrier does
            // not hold them), keeps nine steps of fragments alive and spills ~290 registers
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int jr = 0; jr < NB; ++jr) asm volatile("" : "+v"(acc[mb][jr]) :: "memory");
            if (t + 1 < NKS) __builtin_amdgcn_sched_barrier(0);
        }
        near_end();
    } else if constexpr (X3) {
        // 9 taps x (10 fragment reads, 18 MFMAs): K-step h = 0 holds the hi parts, h = 1 the lo parts of the stage's 16 channels;
        // acc += w_lo.x_hi + w_hi.x_lo + w_hi.x_hi (small terms first).  Fragments of tap s + 1 are fetched while tap s multiplies.
        x3h8 a[2][2][MB], b[2][2][NB];
        // the 2 (MB + NB) fragment reads of a tap in three parts, one per term group of the tap before it (below)
        constexpr int NFR = 2 * (MB + NB);
        auto load_part = [&](int sidx, int buf, int part) __attribute__((always_inline)) {
            const int dy = sidx / 3, dx = sidx - dy * 3;
#pragma unroll
            for (int i = part * NFR / 3; i < (part + 1) * NFR / 3; ++i) {
                const int h = i / (MB + NB), r = i - h * (MB + NB);
                if (r < MB) a[buf][h][r] = *reinterpret_cast<const x3h8*>(aptr + ((2 * sidx + h) * MB + r) * 1024);
                else b[buf][h][r - MB] = *reinterpret_cast<const x3h8*>(bptr[dx][(r - MB + dy + 2 * h) & 3] + (r - MB + dy) * HP * 64);
            }
        };
#pragma unroll
        for (int part = 0; part < 3; ++part) load_part(0, 0, part);
#pragma unroll
        for (int sidx = 0; sidx < NKS; ++sidx) {
            const int cur = sidx & 1;
            if (sidx == NKS - 1) near_end();
            // Term by term over the MB x NB accumulators, NOT three terms per accumulator in a row, and every group fenced: an
            // instruction between two MFMAs on the SAME accumulator costs ~43 clk (MI355X_MICROARCH.md), between MFMAs on different ones
            // ~6 -- and the next tap's fragment reads sit between these MFMAs (left alone, hipcc's scheduler clusters the three
            // MFMAs of an accumulator and drops the reads in between).  Per accumulator the order of the terms is unchanged (small
            // terms first): same bits.
#pragma unroll
            for (int term = 0; term < 3; ++term) {
                constexpr int NR = NFR / 3 + 1;
                if (sidx + 1 < NKS) load_part(sidx + 1, cur ^ 1, term);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int jr = 0; jr < NB; ++jr)
                        acc[mb][jr] = X3_MFMA_32x32x16(a[cur][term == 0 ? 1 : 0][mb], b[cur][term == 1 ? 1 : 0][jr], acc[mb][jr]);
                if (sidx + 1 < NKS) {                          // one fragment read behind each of the group's first MFMAs
#pragma unroll
                    for (int i = 0; i < NR; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, MB * NB - NR, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        // 18 K = 16 steps (tap, channel half) x 6 MFMAs of 32 x 32 x 16; fragments of step t + 1 are fetched while step t
        // multiplies.  `near_end` runs before the last two steps (the token is handed on while ~400 clk of MFMAs are queued).
        bf16x8 a[2][MB], b[2][NB];
        auto load_frags = [&](int t, int buf) {
            const int s = t >> 1, h = t & 1, dy = s / 3, dx = s - dy * 3;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) a[buf][mb] = *reinterpret_cast<const bf16x8*>(aptr + (t * MB + mb) * 1024);
#pragma unroll
            for (int jr = 0; jr < NB; ++jr)
                b[buf][jr] = *reinterpret_cast<const bf16x8*>(bptr[dx][(jr + dy + 2 * h) & 3] + (jr + dy) * HP * 64);
        };
        load_frags(0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int cur = t & 1;
            if (t == NT - 2) near_end();
            if (t + 1 < NT) load_frags(t + 1, cur ^ 1);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int jr = 0; jr < NB; ++jr)
                    acc[mb][jr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[cur][mb], b[cur][jr], acc[mb][jr], 0, 0, 0);
            if (t + 1 < NT) {                                  // one fragment read behind each of the first five MFMAs of the step
#pragma unroll
                for (int i = 0; i < MB + NB; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, MB * NB - (MB + NB), 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// FP8 = false: bf16 operands, v_mfma_f32_32x32x16_bf16, stages of 32 input channels.
// FP8 = true (BASELINE config C5): OCP e4m3 operands -- the input is the e4m3 twin of the activation tensor (per-tensor scale),
// the weights carry one scale per output channel -- on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales: stages of 64
// input channels in the same 54 KB + 22.5 KB of LDS, i.e. half the stages and half the DMA bytes per MAC, twice the MACs per
// matrix-pipe cycle.  y = sum * (input scale x weight scale) + folded-BN shift is applied in the epilogue; the output goes out
// as bf16 and / or as the e4m3 twin the next fp8 convolution reads.
// MODE 2 (X3, the fp32-class engine `bf16x3`): fp32 activations and weights split into bf16 hi + bf16 lo (x = hi + lo to 2^-17),
// y = hi.hi + hi.lo + lo.hi accumulated in fp32 -- three v_mfma_f32_32x32x16_bf16 per product where the exact-fp32 engine's
// v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16 rate.  Measured against the plain fp32 forward (tools/x3_sim.py arithmetic):
// |dlogp| 5e-6 mean / 1.4e-4 max, identical keypoint indices on every row.  The operand tensors are "split twins": per pixel and
// 16-channel group [16 hi | 16 lo] bf16 -- byte for byte a bf16 tensor of 2 C pseudo-channels, so the halo / weight staging of the
// bf16 mode is used unchanged (a stage = 16 real channels); only the MFMA pairing and the fp32 epilogue differ.
template <int MB, int NB, int MODE>
__global__ __launch_bounds__(512, 2) void conv_tt_kernel(const TTParams P) {
    using S = TTShape<MB, NB>;
    constexpr int COUT_BLK = S::COUT_BLK, W_BYTES = S::W_BYTES, HP = S::HP, HROWS = S::HROWS, HALO_PIECES = S::HALO_PIECES, HV = S::HV;
    constexpr int TEAM_BYTES = S::TEAM_BYTES, EPI_PITCH = S::EPI_PITCH, EPI_GROUPS = S::EPI_GROUPS, EPI_ITERS = S::EPI_ITERS;
    constexpr bool FP8 = MODE == 1, X3 = MODE == 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int team = wv >> 2, tw = wv & 3;
    const unsigned T = blockIdx.x * 2u + (unsigned)team;
    char* const s_w = smem + team * TEAM_BYTES;
    char* const s_h = s_w + W_BYTES;
    float* const s_bias = reinterpret_cast<float*>(smem + 2 * TEAM_BYTES + 64);     // folded-BN shifts of the members, back to back
    float* const s_osc = s_bias + TT_TABLE_MAX;                                     // fp8 variant: output scales, same indexing
    const int tab1 = P.m[0].cout, tab2 = P.m[0].cout + P.m[1].cout;                 // table offsets of members 1 and 2

    // Work distribution (round 5: dynamic).  The items of an XCD sit in ONE list, most expensive member first, and a team takes the next
    // one with an atomic on the XCD's counter (P.queue[xcd]); rounds 2-4 dealt every team a fixed list on the host.  The kernel is one
    // workgroup per CU, and a CU that is held when the launch begins -- a camera-solve wavefront of an earlier batch owns a SIMD's whole
    // register file for up to hundreds of milliseconds at the reference's refine criterion -- starts its workgroup only when another one
    // has LEFT: with fixed lists the launch then lasted twice as long, with the queue the late workgroup finds it empty.  Wave 0 of a team
    // grabs two items ahead (atomic -> descriptor load -> LDS slot by item parity, all behind waits the stage needs anyway), the team's
    // other waves read the slot when an item ends.  The last team of an XCD to leave re-arms that XCD's counters (P.queue[8 + xcd] counts its leavers).

    // B fragment of K = 16 step (tap (dy, dx), channel half h) for tile row jr of this wave: pixel (tw * NB + jr + dy, l31 + dx),
    // channel group cg = 2 h + hi, stored in slot (rot + cg) & 3 with rot = (pixel >> 2) & 3 = (row + ((l31 + dx) >> 2)) & 3
    // (row pitch 36 = 9 * 4).  bptr[dx][k] carries everything that depends on the lane for k = (jr + dy + 2 h) & 3; the rest of
    // the address, (jr + dy) * 36 * 64, is an immediate of the ds_read.
    const char* bptr[3][4];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            bptr[dx][k] = s_h + ((tw * NB * HP + l31 + dx) * 64 + ((tw * NB + ((l31 + dx) >> 2) + (FP8 ? 2 * hi : hi) + k) & 3) * 16);
    const char* const aptr = s_w + lane * 16;

    unsigned long long* const trc = P.trace ? P.trace + (size_t)T * 256 : nullptr;
    unsigned tix = 0, eix = 192;          // [0,192): six stamps per stage; [192,255): four stamps per epilogue; [255] finish
    if (trc && tid == team * 256) trc[254] = __builtin_amdgcn_s_memrealtime();
    constexpr bool trace_on = true;       // (rounds 3-4 could stamp a team's LAST 32 stages, SNCAL_TT_ABLATE bit 64: a queue has no known last stage)
    auto stamp = [&]() { if (trc && trace_on && tid == team * 256 && tix < 192) trc[tix++] = __builtin_amdgcn_s_memtime(); };
    auto estamp = [&]() { if (trc && trace_on && tid == team * 256 && eix < 254) trc[eix++] = __builtin_amdgcn_s_memtime(); };

    // ---- state of the team's current item ---------------------------------------------------------------------------
    // Beside a multiplying partner wave, a dependent VALU instruction of the loading wave completes every 5-8 clk and a
    // vector-memory instruction costs ~160 clk (phase traces, tools/tt_trace.py): per-lane address arithmetic and the 24
    // loads / stores of an epilogue are the expensive parts of a LOAD phase.  So the halo offsets are computed once per
    // item (not per stage), and the epilogue's addresses are split into a wave-uniform scalar part (row, tile column,
    // channel block: SALU) and per-lane constants.
    f32x16 acc[MB][NB];
    [[maybe_unused]] float amax = 0.f;     // fp16x3: range tracker of the twin splits (x3.hpp)
    unsigned hv[HV];                       // per-lane byte offsets of this wave's halo DMA pieces (stage-independent)
    TTMember M = load_member(0);
    int nb = 0, c = 0, row0 = 0, col0 = 0, tab = 0;

    // byte offset of this lane's 16 bytes of halo piece `piece`: slot q of the [pixel][4] image holds channel group
    // (q & 3) - (pixel >> 2) mod 4; pitch padding, rows / columns outside the frame and the shared zero row between
    // stacked frames get an out-of-range offset -> the DMA writes zeros.  (Splitting this into per-lane kernel constants and
    // a wave-uniform scalar part per item -- 42 instead of ~200 VALU instructions -- was built and measured SLOWER: the
    // scalar part pushed the kernel over the 102-SGPR budget and the spills cost more than the VALU work saved.)
    auto halo_voff = [&](int piece, int lane) -> unsigned {
        const unsigned q = (unsigned)(piece * 64 + lane);
        const unsigned p = q >> 2;
        const unsigned hrow = (p * 1821u) >> 16, hcol = p - hrow * HP;           // p / 36 for p < 2048
        const unsigned cg = ((q & 3u) - (p >> 2)) & 3u;
        const int s = row0 - 1 + (int)hrow;
        const unsigned f = __umulhi((unsigned)max(s, 0), M.hp1_magic);
        const int y = s - (int)f * (M.H + 1);
        const int x = col0 - 1 + (int)hcol;
        const bool ok = (hrow < (unsigned)HROWS) & (hcol < 34u) & (s >= 0) & ((int)f < M.N) & (y < M.H) & ((unsigned)x < (unsigned)M.W);
        return ok ? (unsigned)((((int)f * M.H + y) * M.W + x) * M.Cin * (FP8 ? 1 : 2)) + cg * 16u : BUF_OOB;
    };

    // (bf16x3: called AFTER the first stage's DMA wait, so that the accumulator registers are free while the residual loads are in flight)
    auto init_acc = [&]() __attribute__((always_inline)) {
        // accumulators start at the folded-BN shift: register quad q of block mb holds channels mb * 32 + 8 q + 4 hi + 0..3 of
        // pixel l31.  The shifts come from a table in LDS (filled once per workgroup): a global load here would sit behind the
        // old tile's stores and its wait, vmcnt(0), would last until every store has drained
        if constexpr (FP8) {               // fp8: plain sums; scale and shift are applied in the epilogue
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int jr = 0; jr < NB; ++jr)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mb][jr][r] = 0.f;
        } else {
            // register quad q of block mb holds channels mb * 32 + 8 q + 4 hi + 0..3; bf16x3: x3_quad_channel(q, hi) (the weight rows are
            // permuted so that quads 2 p and 2 p + 1 of a lane are 8 CONSECUTIVE channels: its 16-byte piece of a split twin)
            const float* const bt = s_bias + tab + nb * COUT_BLK;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 bs = *reinterpret_cast<const float4*>(bt + mb * 32 + (X3 ? x3_quad_channel(q, hi) : 8 * q + 4 * hi));
#pragma unroll
                    for (int jr = 0; jr < NB; ++jr) {
                        acc[mb][jr][4 * q + 0] = bs.x; acc[mb][jr][4 * q + 1] = bs.y; acc[mb][jr][4 * q + 2] = bs.z; acc[mb][jr][4 * q + 3] = bs.w;
                    }
                }
        }
    };
    int cur_m = -1;                        // member of the current item
    auto halo_offsets = [&]() __attribute__((always_inline)) {
        int lane_l = lane;                 // laundered: hipcc would hoist the lane-only parts out of the stage loop and spill them
        asm volatile("" : "+v"(lane_l));
#pragma unroll
        for (int jj = 0; jj < HV; ++jj) hv[jj] = tw + 4 * jj < HALO_PIECES ? halo_voff(tw + 4 * jj, lane_l) : BUF_OOB;
    };
    auto setup_item = [&](const TTItem I) {
        M = load_member(I.member);
        cur_m = I.member;
        nb = I.nb; row0 = I.row0; col0 = I.col0;
        halo_offsets();
        if (eix > 192) estamp();
        tab = I.member == 0 ? 0 : I.member == 1 ? tab1 : tab2;
        if constexpr (!X3) init_acc();
    };

    // bf16x3: the residual of a BasicBlock's second convolution is ADDED INTO THE ACCUMULATORS BEFORE the first multiply instead of in
    // the epilogue.  A phase trace (round 4, tools/tt_trace.py per launch) showed what the epilogue's residual reads cost: 24k clk per tile
    // with them against 10k without (64 x 12 x 32 tile; 33k against 11k on the 96-channel tile) -- every tile row paid an exposed HBM round
    // trip plus 6-12 vector-memory instructions at ~160 clk beside a multiplying partner.  Requested at item set-up, the same loads
    // travel with the first stage's DMA and are covered by the wait that stage needs anyway (s_waitcnt vmcnt(0) below); the unpack
    // (hi + lo of the block input's split twin, or fp32) is ~1 VALU instruction per element in front of the first multiply.  The sum
    // bias + residual + products is the same set of fp32 terms in another order.  Layout: registers 8 p .. 8 p + 7 of a lane are 8
    // consecutive channels (x3_quad_channel), i.e. the lane's 16 bytes of the hi half and of the lo half of 16-channel group 2 mb + p.
    typedef unsigned u32x4r __attribute__((ext_vector_type(4)));
    constexpr int NU = 2 * MB;
    u32x4r rres[X3 ? NB : 1][X3 ? NU : 1][2];
    auto residual_issue = [&]() __attribute__((always_inline)) {
        // BRANCH-FREE inside: the two residual forms (split twin: dense, stride = the layer's width, hi at +0 and lo at +32 bytes of a
        // 64-byte group; fp32: the output's stride, +0 and +16) differ in wave-uniform scalars only, dead channel groups of a padded block
        // and pixels outside the image get an out-of-range offset (the load returns zeros).  With `if`s around the loads hipcc kept the
        // array in scratch and waited for every load on the spot.
        const bool rs = M.res_split != 0;
        const int cstr = rs ? M.cout : M.out_cstride;
        const int coff = rs ? 0 : M.out_coff;
        const int lane_ch = rs ? hi * 4 : hi * 8;                 // in 4-byte units inside the 16-channel group
        const unsigned second = rs ? 32u : 16u;
        const __amdgpu_buffer_rsrc_t rs_res = buf_rsrc(M.res, (int)(unsigned)(M.N * M.H * M.W * cstr * 4));
        const unsigned lane_off = (unsigned)((l31 * cstr + lane_ch) * 4);
#pragma unroll
        for (int jr = 0; jr < (X3 ? NB : 1); ++jr) {
            const int srow = row0 + tw * NB + jr;
            const unsigned f = __umulhi((unsigned)srow, M.hp1_magic);
            const int y = srow - (int)f * (M.H + 1);
            const bool row_ok = ((int)f < M.N) & (y < M.H);
            const bool px_ok = row_ok & (l31 < M.W - col0);
            const unsigned soff = row_ok ? (unsigned)(((((int)f * M.H + y) * M.W + col0) * cstr + coff + nb * COUT_BLK) * 4) : 0u;
#pragma unroll
            for (int u = 0; u < (X3 ? NU : 1); ++u) {
                const bool live = nb * COUT_BLK + u * 16 < M.cout;        // wave-uniform: padded groups of a narrow layer
                const unsigned v = (px_ok & live) ? lane_off + (unsigned)(u * 64) : BUF_OOB;
                rres[jr][u][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, v, soff, 0);
                rres[jr][u][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, v, soff + second, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // accumulators = folded-BN shift (+ residual), one (row, 32-channel block) at a time: the 16 registers of a block are born as the 16
    // residual registers they absorb die (hipcc spills the whole residual array if all accumulators are initialised first)
    auto init_acc_x3 = [&](const bool with_res) __attribute__((always_inline)) {
        const bool rs = M.res_split != 0;
        const float* const bt = s_bias + tab + nb * COUT_BLK;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            float bsv[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bs = *reinterpret_cast<const float4*>(bt + mb * 32 + x3_quad_channel(q, hi));
                bsv[4 * q] = bs.x; bsv[4 * q + 1] = bs.y; bsv[4 * q + 2] = bs.z; bsv[4 * q + 3] = bs.w;
            }
#pragma unroll
            for (int jr = 0; jr < NB; ++jr) {
                f32x16 a;
#pragma unroll
                for (int r = 0; r < 16; ++r) a[r] = bsv[r];
                if (with_res) {
#pragma unroll
                    for (int pq = 0; pq < 2; ++pq) {
                        const u32x4r ra = rres[jr][2 * mb + pq][0], rb = rres[jr][2 * mb + pq][1];
                        if (rs) {                   // split twin: a += lo + hi, the sum of the pair as one v_fma_mix_f32 (x3_join)
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                a[8 * pq + 2 * k] += x3_join<0>(ra[k], rb[k]);
                                a[8 * pq + 2 * k + 1] += x3_join<1>(ra[k], rb[k]);
                            }
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) { a[8 * pq + k] += __uint_as_float(ra[k]); a[8 * pq + 4 + k] += __uint_as_float(rb[k]); }
                        }
                    }
                }
                acc[mb][jr] = a;
            }
        }
    };

    auto setup_done_stamp = [&]() { if (eix > 192) estamp(); };
    auto issue_stage = [&](int cc) {
        const __amdgpu_buffer_rsrc_t rs_in = buf_rsrc(M.in, (int)M.in_bytes);
        const __amdgpu_buffer_rsrc_t rs_w = buf_rsrc(M.w, (int)M.w_bytes);
        // (weights first: requesting the halo pieces first -- they come from HBM / the Infinity Cache, the weights from L2 -- was measured
        // 1.3 % slower on the fp16x3 step, round 4)
        const unsigned wbase = (unsigned)((nb * M.chunks + cc) * W_BYTES);
        const int i1 = S::wp_first(tw + 1);
        for (int i = S::wp_first(tw); i < i1; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_void*)(s_w + i * 1024), 16, (unsigned)(lane * 16), wbase + i * 1024, 0, 0);
        const unsigned cbase = (unsigned)(cc * 64);
#pragma unroll
        for (int jj = 0; jj < HV; ++jj)
            if (tw + 4 * jj < HALO_PIECES) {
                // (a named copy: with hv[jj] -- an array whose bound depends on the template parameters -- as the builtin's argument, hipcc
                // 7.2's HOST pass silently emits no stub for the kernel and the library has an undefined symbol)
                const unsigned voff = hv[jj];
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (lds_void*)(s_h + (tw + 4 * jj) * 1024), 16, voff, cbase, 0, 0);
            }
    };

    // (+ residual) (ReLU) -> bf16, through a wave-private LDS transpose so that every lane stores 8 consecutive channels.
    // BRANCH-FREE: residual loads and output stores go through buffer descriptors, an item with nothing to store carries an
    // out-of-range offset (loads return zeros, stores are dropped), a missing residual is a zero-sized descriptor.  (The
    // first version guarded every 16-byte load with `if (res && valid)`: hipcc then branches around each load and waits for
    // it before the next -- twelve dependent HBM round trips, 12k clk per tile against a 4k clk MFMA phase of the other team.)
    auto epilogue_x3 = [&]() __attribute__((always_inline)) {
        // fp32 in, fp32 out: (+ residual) (ReLU), 8 channels = 32 bytes per lane and item = two b128 accesses each way; channel blocks
        // beyond the layer's width (a 48-channel layer runs as one 96-channel item with zero weights above 48) are not stored
        const unsigned out_bytes = (unsigned)(M.N * M.H * M.W * M.out_cstride * 4);
        const __amdgpu_buffer_rsrc_t rs_out = buf_rsrc(M.out ? M.out : M.in, M.out ? (int)out_bytes : 0);
        // split twin of the output for the next bf16x3 convolution ([16 hi | 16 lo] bf16 per 16-channel group: 4 bytes per element like
        // the fp32 tensor; written here the consumer needs no separate split pass).  Twin tensors are dense: stride = the layer's width.
        const unsigned twin_bytes = (unsigned)(M.N * M.H * M.W * M.cout * 4);
        const __amdgpu_buffer_rsrc_t rs_tw = buf_rsrc(M.out8 ? M.out8 : M.in, M.out8 ? (int)twin_bytes : 0);
        const bool has_twin = M.out8 != nullptr;
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const bool narrow48 = COUT_BLK == 64 && M.cout - nb * COUT_BLK == 48;        // wave-uniform
        const bool twin_only = has_twin && M.out == nullptr && !(P.ablate & 32);     // (SNCAL_TT_ABLATE bit 32: always the transposed path)
        const float lob = x3_lower(M.relu != 0);
        estamp();
        int lane_l = lane;
        asm volatile("" : "+v"(lane_l));
        float* const stg = reinterpret_cast<float*>(s_w + S::wp_first(tw) * 1024);
        estamp();
#pragma unroll
        for (int jr = 0; jr < NB; ++jr) {
            const int srow = row0 + tw * NB + jr;
            const unsigned f = __umulhi((unsigned)srow, M.hp1_magic);
            const int y = srow - (int)f * (M.H + 1);
            const bool row_ok = ((int)f < M.N) & (y < M.H);
            const unsigned soff = row_ok ? (unsigned)(((((int)f * M.H + y) * M.W + col0) * M.out_cstride + M.out_coff + nb * COUT_BLK) * 4) : 0u;
            const unsigned soff_tw = row_ok ? (unsigned)(((((int)f * M.H + y) * M.W + col0) * M.cout + nb * COUT_BLK) * 4) : 0u;
            if (jr == 1) estamp();
            if (twin_only) {
                // Inside a BasicBlock chain only the split twin is written: straight from the accumulators.  With the permuted rows a
                // lane's registers 8 p .. 8 p + 7 of block mb are 8 consecutive channels of pixel l31 = its 16 bytes of the hi half and its
                // 16 bytes of the lo half of 16-channel group 2 mb + p; the two lane halves complete each 32-byte half -- the same 32-byte
                // pieces the transposed path writes, without the LDS round trip and its index arithmetic.  (The residual is in the
                // accumulators already: residual_issue / residual_add.)
                const bool px_ok = row_ok & (l31 < M.W - col0);
                constexpr int NU = 2 * MB;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    if (!(nb * COUT_BLK + u * 16 < M.cout)) continue;
                    const int mb = u >> 1, pq = u & 1;
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = acc[mb][jr][8 * pq + k];
                    u32x4 t0, t1;
                    x3_split8(v, lob, t0, t1, amax);        // (ReLU is the split's lower clamp bound)
                    const unsigned vt = px_ok ? (unsigned)(l31 * M.cout * 4 + u * 64 + hi * 16) : BUF_OOB;
                    asm volatile("" : "+v"(t0), "+v"(t1));
                    __builtin_amdgcn_raw_buffer_store_b128(t0, rs_tw, vt, soff_tw, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(t1, rs_tw, vt, soff_tw + 32u, 0);
                    asm volatile("s_nop 3" :: "v"(t0), "v"(t1) : "memory");
                }
                continue;
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(stg + l31 * EPI_PITCH + mb * 32 + x3_quad_channel(q, hi)) =
                        make_float4(acc[mb][jr][4 * q], acc[mb][jr][4 * q + 1], acc[mb][jr][4 * q + 2], acc[mb][jr][4 * q + 3]);
#pragma unroll
            for (int e = 0; e < EPI_ITERS; ++e) {
                // a 48-channel layer in a 64-channel block: 32 pixels x 6 real groups = three rounds of 64 lanes instead of four
                if (narrow48 && e * 64 >= 32 * 6) continue;
                const int id = e * 64 + lane_l;
                const int px = narrow48 ? id / 6 : id / EPI_GROUPS, grp = id - px * (narrow48 ? 6 : EPI_GROUPS);
                const bool ok = row_ok & (px < M.W - col0) & (nb * COUT_BLK + grp * 8 < M.cout);
                const unsigned voff = ok ? (unsigned)((px * M.out_cstride + grp * 8) * 4) : BUF_OOB;
                const float* sp = stg + px * EPI_PITCH + grp * 8;
                const float4 lo = *reinterpret_cast<const float4*>(sp), hi4 = *reinterpret_cast<const float4*>(sp + 4);
                float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
                const unsigned voff_tw = ok ? (unsigned)(px * M.cout * 4 + (grp >> 1) * 64 + (grp & 1) * 16) : BUF_OOB;
                if (M.relu) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
                }
#pragma unroll
                for (int k = 0; k < 8; k += 2) x3_track(amax, v[k], v[k + 1]);       // every OUTPUT is tracked where it is produced (x3.hpp)
                u32x4 o0 = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
                u32x4 o1 = {__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7])};
                // hipcc leaves ONE wait state between a 16-byte store and the next write of its data registers (it reused the first data
                // register of store 1 as the address of store 2, and rewrote store 2's data right behind it); under memory load gfx950
                // reads store data later than that: isolated elements came out holding address bit patterns (the fp8 epilogue below met
                // the same).  So: both vectors complete in registers of their own, no VALU between the stores (the +16 rides in the
                // scalar offset), and the data registers stay live and untouched for four more wait states.
                asm volatile("" : "+v"(o0), "+v"(o1));
                __builtin_amdgcn_raw_buffer_store_b128(o0, rs_out, voff, soff, 0);
                __builtin_amdgcn_raw_buffer_store_b128(o1, rs_out, voff, soff + 16u, 0);
                asm volatile("s_nop 3" :: "v"(o0), "v"(o1) : "memory");
                if (has_twin) {                  // wave-uniform: hi = rne16(y), lo = rne16(y - hi), 16 bytes each, lo 32 bytes behind hi
                    u32x4 t0, t1;
                    x3_split8(v, x3_lower(false), t0, t1);       // (v is past the ReLU already)
                    asm volatile("" : "+v"(t0), "+v"(t1));
                    __builtin_amdgcn_raw_buffer_store_b128(t0, rs_tw, voff_tw, soff_tw, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(t1, rs_tw, voff_tw, soff_tw + 32u, 0);
                    asm volatile("s_nop 3" :: "v"(t0), "v"(t1) : "memory");
                }
            }
        }
        estamp();
    };
    auto epilogue = [&]() __attribute__((always_inline)) {
        if (P.ablate & 1) return;
        if constexpr (X3) { epilogue_x3(); return; }
        const unsigned out_bytes = (unsigned)(M.N * M.H * M.W * M.out_cstride * 2);
        const __amdgpu_buffer_rsrc_t rs_out8 = buf_rsrc(FP8 && M.out8 ? M.out8 : M.in, FP8 && M.out8 ? (int)(out_bytes / 2) : 0);
        const __amdgpu_buffer_rsrc_t rs_res = buf_rsrc(M.res ? M.res : M.in, M.res ? (int)out_bytes : 0);
        const __amdgpu_buffer_rsrc_t rs_out = buf_rsrc(M.out ? M.out : M.in, M.out ? (int)out_bytes : 0);     // no bf16 output: zero-sized
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const bool has_res = M.res != nullptr;      // the first conv of a BasicBlock has none: no loads, no unpack / add (a VALU
        estamp();                                   // instruction beside a multiplying partner costs ~8 clk, a load ~160)
        // item e of a tile row: lane -> pixel px of the row's 32 and 8-channel group grp (lane constants of the kernel)
        int lane_l = lane;
        asm volatile("" : "+v"(lane_l));
        unsigned lane_off[EPI_ITERS];
        int px_e[EPI_ITERS];
#pragma unroll
        for (int e = 0; e < EPI_ITERS; ++e) {
            const int id = e * 64 + lane_l;
            const int px = id / EPI_GROUPS, grp = id - px * EPI_GROUPS;
            px_e[e] = px;
            lane_off[e] = (unsigned)((px * M.out_cstride + grp * 8) * 2);
        }
        u32x4 rr[NB][EPI_ITERS];
        unsigned voff[NB][EPI_ITERS], soff[NB];
#pragma unroll
        for (int jr = 0; jr < NB; ++jr) {
            // wave-uniform part (SALU): stacked row -> (frame, row), channel block
            const int srow = row0 + tw * NB + jr;
            const unsigned f = __umulhi((unsigned)srow, M.hp1_magic);
            const int y = srow - (int)f * (M.H + 1);
            const bool row_ok = ((int)f < M.N) & (y < M.H);
            soff[jr] = row_ok ? (unsigned)(((((int)f * M.H + y) * M.W + col0) * M.out_cstride + M.out_coff + nb * COUT_BLK) * 2) : 0u;
#pragma unroll
            for (int e = 0; e < EPI_ITERS; ++e) {
                voff[jr][e] = (row_ok & (px_e[e] < M.W - col0)) ? lane_off[e] : BUF_OOB;      // out of range: loads 0, stores nothing
                rr[jr][e] = u32x4{0u, 0u, 0u, 0u};
                if (has_res) rr[jr][e] = __builtin_amdgcn_raw_buffer_load_b128(rs_res, voff[jr][e], soff[jr], 0);     // wave-uniform branch
            }
        }
        float* const stg = reinterpret_cast<float*>(s_w + S::wp_first(tw) * 1024);      // this wave's own block of the weight region
        estamp();
#pragma unroll
        for (int jr = 0; jr < NB; ++jr) {
            if (jr == 1) estamp();
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4*>(stg + l31 * EPI_PITCH + mb * 32 + 8 * q + 4 * hi) =
                        make_float4(acc[mb][jr][4 * q], acc[mb][jr][4 * q + 1], acc[mb][jr][4 * q + 2], acc[mb][jr][4 * q + 3]);
            // wave-local hand-off: the LDS operations of one wave complete in order
#pragma unroll
            for (int e = 0; e < EPI_ITERS; ++e) {
                const float* sp = stg + (lane_off[e] >> 1) - px_e[e] * (M.out_cstride - EPI_PITCH);     // px * PITCH + grp * 8
                const float4 lo = *reinterpret_cast<const float4*>(sp), hi4 = *reinterpret_cast<const float4*>(sp + 4);
                float v[8] = {lo.x, lo.y, lo.z, lo.w, hi4.x, hi4.y, hi4.z, hi4.w};
                if constexpr (FP8) {             // y = sum * (input scale x weight scale of the channel) + folded-BN shift
                    __builtin_amdgcn_sched_barrier(0);       // (hipcc hoists the table reads of all twelve items otherwise: 190 registers)
                    const int ch = tab + nb * COUT_BLK + (int)(lane_off[e] >> 1) - px_e[e] * M.out_cstride;      // ... + grp * 8
                    const float4 s0 = *reinterpret_cast<const float4*>(s_osc + ch), s1 = *reinterpret_cast<const float4*>(s_osc + ch + 4);
                    const float4 b0 = *reinterpret_cast<const float4*>(s_bias + ch), b1 = *reinterpret_cast<const float4*>(s_bias + ch + 4);
                    const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, bi[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = v[k] * sc[k] + bi[k];
                }
                if (has_res) {
                    const bf16x8 r = __builtin_bit_cast(bf16x8, rr[jr][e]);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] += (float)r[k];
                }
                bf16x8 q;
#pragma unroll
                for (int k = 0; k < 8; ++k) q[k] = (__bf16)v[k];
                if (M.relu) {       // relu(round(x)) == round(relu(x)); a negative bf16 is a negative int16
                    typedef short s16x8 __attribute__((ext_vector_type(8)));
                    const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                    q = __builtin_bit_cast(bf16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, q), z));
                }
                if constexpr (FP8) {             // e4m3 twin for the next fp8 convolution: the ROUNDED bf16 value / scale, saturated.
                    // Packed BEFORE the bf16 store is issued: with the conversion after it, v_cvt_pk_fp8_f32 was allocated the
                    // store's first data register and, under memory load, overwrote it before the store had read it -- isolated
                    // wrong bf16 elements (first of an 8-channel group, magnitudes of fp8 codes), traced with per-launch checksums.
                    float w8[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) w8[k] = fminf(fmaxf((float)q[k] * M.out8_inv_scale, -448.f), 448.f);
                    int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(w8[0], w8[1], 0, false);
                    p0 = __builtin_amdgcn_cvt_pk_fp8_f32(w8[2], w8[3], p0, true);
                    int p1 = __builtin_amdgcn_cvt_pk_fp8_f32(w8[4], w8[5], 0, false);
                    p1 = __builtin_amdgcn_cvt_pk_fp8_f32(w8[6], w8[7], p1, true);
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const unsigned v8 = voff[jr][e] == BUF_OOB ? BUF_OOB : voff[jr][e] >> 1;
                    u32x4 qd = __builtin_bit_cast(u32x4, q);
                    u32x2 pd = u32x2{(unsigned)p0, (unsigned)p1};
                    asm volatile("" : "+v"(qd), "+v"(pd));      // both packs are complete, in registers of their own, before either store
                    __builtin_amdgcn_raw_buffer_store_b128(qd, rs_out, voff[jr][e], soff[jr], 0);
                    __builtin_amdgcn_raw_buffer_store_b64(pd, rs_out8, v8, soff[jr] >> 1, 0);
                    asm volatile("s_nop 1" ::: "memory");        // ... and two wait states before anything may reuse the data registers
                } else {
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q), rs_out, voff[jr][e], soff[jr], 0);
                }
            }
        }
        estamp();
    };

    // Both teams run the same program -- per stage: LOAD (DMA, and at an item boundary the previous tile's epilogue), team
    // barrier, take the CU's MULTIPLY token, 108 MFMAs per wave, release.  The token makes the MFMA phases of the two teams
    // mutually exclusive (two multiplying waves on one SIMD would only halve each other), so the teams alternate by
    // themselves: while one multiplies the other loads.  They are NOT locked phase by phase: the first version closed every
    // phase with one s_barrier over both teams, and a team whose LOAD phase carried an epilogue (~6k clk: 24 vector-memory
    // instructions per wave at ~160 clk each beside a multiplying partner) held the partner's next multiply back by 2-5k
    // clk per tile.  Now the partner takes the token again as soon as its own next stage has landed.
    // Team-level synchronisation goes through LDS words (one wave-instruction each way, s_sleep while polling):
    //   arrive += 1 per wave when its DMA pieces have landed            go    = k + 1 once wave 0 holds the token
    //   early  += 1 per wave two K-steps before the end of its MFMAs;   the last one frees the token
    //   done   += 1 per wave when its MFMAs (and LDS reads) are over:   the stage's buffers may be overwritten
    unsigned* const ctrl = reinterpret_cast<unsigned*>(smem + 2 * TEAM_BYTES);       // [0] token, [4 + 4 team + {0,1,2,3}] arrive, go, done, early
    unsigned* const w_token = ctrl;
    unsigned* const w_arrive = ctrl + 4 + 4 * team;
    unsigned* const w_go = w_arrive + 1;
    unsigned* const w_done = w_arrive + 2;
    unsigned* const w_early = w_arrive + 3;
    if (tid < 16) ctrl[tid] = 0u;
    for (int i = tid; i < 2 * TT_TABLE_MAX; i += 512) s_bias[i] = 0.f;      // (rows of a padded channel block read table slots nobody fills)
    __syncthreads();
#pragma unroll
    for (int m = 0; m < TT_MAX_MEMBERS; ++m) {
        const int o = m == 0 ? 0 : m == 1 ? tab1 : tab2;
        if (P.m[m].bias && tid < P.m[m].cout) {
            s_bias[o + tid] = P.m[m].bias[tid];
            if constexpr (FP8) s_osc[o + tid] = P.m[m].oscale[tid];
        }
    }
    __syncthreads();
    // The next item's descriptor is fetched ahead (a load that misses every cache: 2-3k clk if waited for on the spot) and published
    // right behind the first stage's own DMA wait (`q_advance`): picking it up at the tile boundary instead meant
    // s_waitcnt vmcnt(0) there -- gfx9 counts stores in vmcnt -- i.e. a full drain of the finished tile's stores in front of the set-up.
    auto item_to_sgprs = [&](const TTItem& I) -> TTItem {
        unsigned d[4];
        __builtin_memcpy(d, &I, 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = (unsigned)__builtin_amdgcn_readfirstlane((int)d[i]);
        TTItem r;
        __builtin_memcpy(&r, d, 16);
        return r;
    };
    // descriptor slots of the team in LDS (the tail of the scale table's region, which no mode fills that far), 16 bytes each; pad_ = 1
    // marks a valid item.
    // A TICKET IS A PAIR OF ITEMS, one for each team of the workgroup: ticket T of the XCD's counter = items 2 T and 2 T + 1 of the XCD's
    // list (tile-major, n-blocks adjacent: mostly two n-blocks of ONE tile, or two neighbouring tiles).  Team 0's wave 0 draws the tickets
    // and publishes both teams' descriptors; team 1 only consumes.  Why pairs: the two teams of a workgroup load in strict alternation
    // (one multiplies while the other loads), so a pair's common halo lines are fetched from HBM once and hit the L2 half a stage later --
    // what round 4's static deal had by construction.  With one ticket per team the n-blocks of a tile went to teams anywhere on the XCD
    // whose stage clocks drift apart over the 12 stages of an item: FETCH_SIZE rose from 310 to 412 MB per grouped launch and the launch
    // took 3 % longer.  The teams of a workgroup stay within one item of each other: team 0 overwrites a slot only when team 1 has started
    // the item before (q_got1), team 1 starts an item when team 0 has published it (q_pub).
    static_assert(4 * sizeof(TTItem) <= TT_QUEUE_FLOATS * sizeof(float), "the queue's four descriptor slots live in the table's last TT_QUEUE_FLOATS floats (hosts admit couts <= TT_COUT_MAX)");
    TTItem* const q_slot = reinterpret_cast<TTItem*>(s_osc + TT_TABLE_MAX - TT_QUEUE_FLOATS) + 2 * team;
    TTItem* const q_slot1 = reinterpret_cast<TTItem*>(s_osc + TT_TABLE_MAX - TT_QUEUE_FLOATS) + 2;      // team 1's slots (written by team 0's wave 0)
    unsigned* const q_pub = ctrl + 1;                             // pairs published so far
    unsigned* const q_got1 = ctrl + 2;                            // pairs team 1 has taken over (all four waves have read the slot)
    const unsigned q_xcd = blockIdx.x & 7u;
    const unsigned q_base = P.xcd_first[q_xcd], q_n = P.xcd_first[q_xcd + 1u] - q_base, q_last = max(q_n, 1u) - 1u;
    auto q_grab = [&]() -> unsigned {                             // (lane 0's value counts; consumed one item later)
        unsigned r = 0;
        if (lane == 0) r = __hip_atomic_fetch_add(P.queue + q_xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return r;
    };
    const bool grabber = team == 0 && tw == 0;
    // The grabber holds ONE pair ahead of the one being multiplied, and fetches it in three steps, each behind a stage's own DMA wait of
    // the current item (`q_step`: nothing of it is waited for on the spot): first stage -- draw the ticket (an atomic on the XCD's counter,
    // ~2 us round trip); next stage -- request the two descriptors (loads that miss every cache: 2-3k clk); the stage after -- publish
    // them to both teams.  Items of fewer than three stages finish the steps at the item's end, waiting.
    // Depth matters at the END of a launch: what a workgroup holds nobody else can take.  A first version held three pairs ahead (ticket,
    // descriptors, published -- one step per ITEM): at batch 64 that is 3 of a workgroup's ~7.6 pairs dealt statically whatever the
    // workgroup's pace, +3 % on the grouped launch against round 4's static longest-first deal; at batch 1 (about one pair per workgroup)
    // the first third of the workgroups to arrive took everything: 5.6 -> 12.3 ms of two-team launches per forward.
    // P.lazy (set by the host when the launch holds fewer than 1.5 pairs per workgroup): not even that one -- the next pair is drawn when
    // the current one is done, its latency (~4 us) exposed, where it is noise.
    const bool lazy = P.lazy != 0;
    unsigned q_pend = 0;                                          // the drawn ticket (lane 0's value; in flight until the next step)
    unsigned q_state = 0;                                         // 0 nothing drawn for the next pair, 1 ticket drawn, 2 descriptors requested, 3 published
    bool q_next_valid0 = false, q_next_valid1 = false;
    TTItem I_next = P.items[q_base], I_next1 = P.items[q_base];
    unsigned q_k = 1;                                             // items this team has started or is about to start
    auto q_request = [&]() __attribute__((always_inline)) {
        const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)q_pend);
        q_next_valid0 = 2u * t < q_n;
        q_next_valid1 = 2u * t + 1u < q_n;
        I_next = P.items[q_base + min(2u * t, q_last)];
        I_next1 = P.items[q_base + min(2u * t + 1u, q_last)];
        q_state = 2;
    };
    auto q_publish = [&]() __attribute__((always_inline)) {
        spin_until(q_got1, q_k - 1u);                             // team 1 has taken over pair q_k - 2: its slot (same parity) may be overwritten
        TTItem d0 = item_to_sgprs(I_next), d1 = item_to_sgprs(I_next1);
        d0.pad_ = q_next_valid0 ? 1 : 0;
        d1.pad_ = q_next_valid1 ? 1 : 0;
        if (lane == 0) { q_slot[q_k & 1u] = d0; q_slot1[q_k & 1u] = d1; }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(q_pub, q_k + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        q_state = 3;
    };
    auto q_step = [&](bool first) __attribute__((always_inline)) {
        if (!grabber) return;
        if (q_state == 0) {
            if (first && !lazy) { q_pend = q_grab(); q_state = 1; }
        } else if (q_state == 1) {
            q_request();
        } else if (q_state == 2) {
            q_publish();
        }
        asm volatile("" ::: "memory");
    };
    if (grabber) {                                                // the workgroup's first pair
        q_pend = q_grab();
        q_request();
        q_k = 0;
        q_publish();                                              // (q_got1 = 0 >= -1; slot 0; q_pub = 1)
        q_k = 1;
        q_state = 0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    TTItem I_ready = item_to_sgprs(q_slot[0]);
    bool have = I_ready.pad_ != 0;
    unsigned st = 0;
    for (; have; ++st) {
        stamp();                                                  // [0] LOAD begins
        if (c == 0) {
            // bf16x3 / fp16x3, next tile of the SAME convolution behind a twin-only epilogue (it stores straight from the accumulators: no
            // LDS staging): the new tile's first stage is requested BEFORE the finished tile is written out.  The team's buffers are free
            // (everyone is done with the last stage), the member's parameters stay, and the halo's HBM latency (2-5k clk, exposed behind the
            // epilogue until now) runs under the epilogue's ~6k clk of splits and stores.  Consecutive items of a team are mostly of one
            // member (the planner deals them longest first).
            bool early = false;
            if constexpr (X3) {
                if (st > 0 && (int)I_ready.member == cur_m && M.out8 != nullptr && M.out == nullptr && !(P.ablate & (1 | 4 | 32))) {
                    const int nb_o = nb, row0_o = row0, col0_o = col0;
                    nb = I_ready.nb; row0 = I_ready.row0; col0 = I_ready.col0;
                    halo_offsets();
                    issue_stage(0);
                    const int nb_n = nb, row0_n = row0, col0_n = col0;
                    nb = nb_o; row0 = row0_o; col0 = col0_o;
                    epilogue();
                    nb = nb_n; row0 = row0_n; col0 = col0_n;
                    early = true;
                }
            }
            if (st > 0 && !early) epilogue();                     // the finished tile, out of registers that the new one needs
            if constexpr (X3) {                                   // the old tile is out: tell the compiler that its registers are free
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int jr = 0; jr < NB; ++jr) acc[mb][jr] = __builtin_nondeterministic_value(acc[mb][jr]);
            }
            if (!early) setup_item(I_ready);
            setup_done_stamp();
            if constexpr (X3) {
                // one straight path from the old tile's epilogue to the new accumulators: between them the accumulator registers are dead
                // and hold the residual while it is in flight (two copies of the path, with and without residual: no phis on the array)
                if (M.res != nullptr && !(P.ablate & 1)) {
                    residual_issue();
                    stamp();                                      // [1] epilogue / setup done
                    if (!(P.ablate & 4) && !early) issue_stage(0);
                    stamp();                                      // [2] DMA issued
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my DMA pieces and the residual have landed (and my stores are out)
                    q_step(true);
                    init_acc_x3(true);
                } else {
                    stamp();
                    if (!(P.ablate & 4) && !early) issue_stage(0);
                    stamp();
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    q_step(true);
                    init_acc_x3(false);
                }
            }
        }
        if (!X3 || c != 0) {
            stamp();                                              // [1] epilogue / setup done
            if (!(P.ablate & 4)) issue_stage(c);
            stamp();                                              // [2] DMA issued
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my DMA pieces have landed (and my stores are out)
            // (fp16x3, round 4: prefetching the NEXT stage's halo lines behind an odd stage's DMA -- one dword per lane by LDS-DMA into an
            // unused LDS region, vmcnt(5) instead of vmcnt(0) -- measured 1.5 % slower: 33.1 against 32.6 ms per step)
            q_step(c == 0);
        }
        stamp();                                                  // [3] landed
        if (lane == 0) __hip_atomic_fetch_add(w_arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (tw == 0) {
            spin_until(w_arrive, 4u * (st + 1u));                 // the whole stage is in LDS
            if (team == 1 && c == 0 && lane == 0)                 // (first stage of an item: all four waves have read this item's slot)
                __hip_atomic_store(q_got1, q_k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            for (;;) {                                            // take the token
                unsigned got = 0;
                if (lane == 0) {
                    unsigned expect = 0u;
                    got = __hip_atomic_compare_exchange_strong(w_token, &expect, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ? 1u : 0u;
                }
                if (__builtin_amdgcn_readfirstlane(got)) break;
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane == 0) __hip_atomic_store(w_go, st + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else {
            spin_until(w_go, st + 1u);
        }
        asm volatile("" ::: "memory");
        stamp();                                                  // [4] MULTIPLY begins
        if (P.ablate & 2) {
            unsigned old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(w_early, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (lane == 0 && old == 4u * st + 3u) __hip_atomic_store(w_token, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else
        tt_multiply_stage<MB, NB, MODE>(acc, aptr, bptr, [&]() {
            unsigned old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(w_early, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (lane == 0 && old == 4u * st + 3u) __hip_atomic_store(w_token, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stamp();                                                  // [5] MFMAs issued
        if (lane == 0) __hip_atomic_fetch_add(w_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        spin_until(w_done, 4u * (st + 1u));                       // every wave of the team is done reading this stage
        if (++c == M.chunks) {                                    // the item is multiplied: the team's next one (published during this one), or none
            c = 0;
            if (grabber) {                                        // whatever is left of the next pair's three steps (lazy: all of them), waiting
                if (q_state == 0) { q_pend = q_grab(); q_state = 1; }
                if (q_state == 1) q_request();
                if (q_state == 2) q_publish();
                q_state = 0;
            } else {
                spin_until(q_pub, q_k + 1u);
            }
            I_ready = item_to_sgprs(q_slot[q_k & 1u]);
            have = I_ready.pad_ != 0;
            ++q_k;
        }
    }
    if (st > 0) epilogue();
    if constexpr (X3) x3_report(amax, P.range);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // (wave 0: its last ticket has come back as well)
    // the per-XCD form of ticket_leave (persist.hpp), at agent scope:
    // the leavers are counted per XCD (32 atomics on an address at the end of a launch, not 512); the last workgroup of an XCD re-arms that
    // XCD's two words for the next launch on this stream: every grabber of the XCD holds its failing tickets and has left the queue
    const unsigned q_wgs = (gridDim.x - q_xcd + 7u) / 8u;         // (only team 0's wave 0 draws tickets: workgroups are counted)
    if (tid == 0 && __hip_atomic_fetch_add(P.queue + 8 + q_xcd, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == q_wgs - 1u) {
        __hip_atomic_store(P.queue + q_xcd, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(P.queue + 8 + q_xcd, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (trc && tid == team * 256) trc[255] = __builtin_amdgcn_s_memrealtime();      // the team's finish time, 100 MHz chip-wide clock (tools/tt_finish.py)
}

}  // namespace sncal
