// Fused HRNet head, 32 x 32 x 16 MFMA version (bf16 path; keypoint network: two gathered wide branches, K1 a multiple of 16).
//
// Same mathematics and the same restructuring as head.hip (read its header first):
//     stage 1  MFMA   h = W0_d . [direct | up(narrow branches)]                      (K1 = 64 + 48 + 96 = 208)
//     gather   MFMA   h += sum_s t_s . wint_s      t_s = box pixels of the wide branch's product at native resolution,
//                                                   wint_s = this output pixel's bilinear weights over the box (B fragment)
//              VALU   h = relu(h)                  (the folded-BN shift is stage 1's initial value)
//     stage 2  MFMA   logits += W1[:, 32-slice] . h
// for /root/reference/src/models/hrnet/hrnet.py:489-510, :316-329.  What changes is the tiling: a wave owns 32 pixels of one
// output row and every product is a v_mfma_f32_32x32x16_bf16 -- 32 hidden channels x 32 pixels per instruction.  Against the
// 16 x 16 x 32 version per 32 pixels and 32-channel slice: 19 MFMAs of 32 clk instead of 40 of ~19.4, 17 A-fragment reads from
// LDS instead of 36 (the fused head was LDS-bound after its gather moved to the matrix pipe), and a workgroup's slice of
// weights (17 KB of LDS-DMA) serves 128 pixels instead of 64.
// The hand-off between the two GEMMs is still a register repack: MFMA row r of a 32-row block carries channel
// h32_row_channel(r) (head.hpp), so registers 8 h .. 8 h + 7 of a lane's accumulator are the channels 16 h + 8 (lane >> 5) + 0..7
// of its pixel -- exactly the 8 k-values that lane must supply to stage 2's K = 16 step h.
#include "persist.hpp"
#include "head.hpp"
#include "softmax_px.hpp"

#pragma clang fp contract(fast)
#include "head_frame.hpp"

namespace sncal {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int H32_SRC = 8 * 1024;          // per slice buffer: 4 waves x 2 sources x one 1 KB DMA piece (16 box pixels x 64 B)

// Single-buffered slices: 26 KB of LDS and 128 VGPRs let FOUR workgroups share a CU, and a workgroup's prologue (boxes, interpolation
// weights, 13 B fragments: 22 % of its life) and slice waits hide under the others -- 3.8 ms against 4.2 ms double-buffered at three
template <int RB, int KS, int DEC>
__global__ __launch_bounds__(256, 4) void head32_kernel(const HeadParams p) {
    constexpr int OFF_W0 = H32_SRC, OFF_W1 = OFF_W0 + KS * 1024, OFF_B0 = OFF_W1 + RB * 2 * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned long long t_begin = p.trace ? __builtin_amdgcn_s_memtime() : 0ull;
    const HeadTile tl = head_tile(p, 32, 4);
    const int n = tl.n, oy0 = tl.oy0, ox0 = tl.ox0;
    const int y = oy0 + wave, yc = min(y, p.H - 1);
    const int x = ox0 + l31, xc = min(x, p.W - 1);
    const bool valid = y < p.H && x < p.W;
    const long pix = ((long)n * p.H + yc) * p.W + xc;

    // ---- this wave's source boxes (its row, its 32 columns) and its two DMA pieces per slice -------------------------------------
    unsigned dma_voff[2][1];
    bf16x8 wint[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        // the B fragment of the interpolation GEMM holds the same bf16 weights as head.hip's
        HeadBoxTaps b = head_box32<2, 1>(p, s, ox0, yc, xc, lane, dma_voff[s]);
        b.w00 = (float)(__bf16)b.w00; b.w01 = (float)(__bf16)b.w01; b.w10 = (float)(__bf16)b.w10; b.w11 = (float)(__bf16)b.w11;
#pragma unroll
        for (int e = 0; e < 8; ++e) wint[s][e] = (__bf16)head_box_weight(b, 8 * hi + e);
    }

    // everything the slice loop consumes comes through LDS-DMA (an ordinary global load inside the loop would make hipcc wait
    // vmcnt(0) at its first use and drain the prefetch every iteration)
    const __amdgpu_buffer_rsrc_t rs_w0 = buf_rsrc(p.w0_32, p.NQ * KS * 1024);
    const __amdgpu_buffer_rsrc_t rs_w1 = buf_rsrc(p.w1_32, p.NQ * RB * 2 * 1024);
    const __amdgpu_buffer_rsrc_t rs_b0 = buf_rsrc(p.bias0, p.HP * 4);
    __amdgpu_buffer_rsrc_t rs_src[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const size_t img = (size_t)p.Hs[s] * p.Ws[s] * p.HP * 2;      // one image of source s (ranges stay < 2 GB)
        rs_src[s] = buf_rsrc(reinterpret_cast<const char*>(p.src[s]) + (size_t)n * img, (int)img);
    }
    auto issue_slice = [&](int q) {
        char* const base = smem;
#pragma unroll
        for (int s = 0; s < 2; ++s)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src[s], (lds_void*)(base + (wave * 2 + s) * 1024), 16, dma_voff[s][0], (unsigned)(q * 64), 0, 0);
#pragma unroll
        for (int i = 0; i < (KS + 3) / 4; ++i)
            if (wave + 4 * i < KS)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w0, (lds_void*)(base + OFF_W0 + (wave + 4 * i) * 1024), 16, (unsigned)(lane * 16),
                                                         (unsigned)((q * KS + wave + 4 * i) * 1024), 0, 0);
        if (wave < RB * 2)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (lds_void*)(base + OFF_W1 + wave * 1024), 16, (unsigned)(lane * 16),
                                                     (unsigned)((q * RB * 2 + wave) * 1024), 0, 0);
        if (wave == 3)      // 32 shift values = 128 B; the other lanes read out of range
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_b0, (lds_void*)(base + OFF_B0), 16,
                                                     lane < 8 ? (unsigned)(lane * 16) : BUF_OOB, (unsigned)(q * 128), 0, 0);
    };
    issue_slice(0);

    // ---- stage-1 B fragments: K = [direct channels | upsampled narrow branches]; lane (pixel l31, k-block hi) holds channels
    // 16 ks + 8 hi .. + 7.  Segment boundaries are multiples of 8 channels, so a lane's k-group lies in exactly one segment.
    bf16x8 bD[KS];
    const __bf16* direct = reinterpret_cast<const __bf16*>(p.direct);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int kk = ks * 16 + hi * 8;
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kk < p.Cd) {
            v = *reinterpret_cast<const bf16x8*>(direct + pix * p.Cd + kk);
        } else {
            int seg0 = p.Cd;
#pragma unroll
            for (int f = 0; f < HEAD_MAX_FOLD; ++f) {
                if (f < p.nfold) {
                    if (kk >= seg0 && kk < seg0 + p.Cf[f]) {
                        const HeadTap tp = head_tap(p.fsy[f], p.fsx[f], p.Hf[f], p.Wf[f], yc, xc);
                        const float ly1 = tp.ly1, lx1 = tp.lx1;
                        const int dx = tp.more_x ? p.Cf[f] : 0, dy = tp.more_y ? p.Wf[f] * p.Cf[f] : 0;
                        const __bf16* t = reinterpret_cast<const __bf16*>(p.fold[f]) +
                                          (((size_t)n * p.Hf[f] + tp.iy) * p.Wf[f] + tp.ix) * p.Cf[f] + (kk - seg0);
                        const bf16x8 t00 = *reinterpret_cast<const bf16x8*>(t), t01 = *reinterpret_cast<const bf16x8*>(t + dx);
                        const bf16x8 t10 = *reinterpret_cast<const bf16x8*>(t + dy), t11 = *reinterpret_cast<const bf16x8*>(t + dy + dx);
                        const float w00 = (1.f - lx1) * (1.f - ly1), w01 = lx1 * (1.f - ly1), w10 = (1.f - lx1) * ly1, w11 = lx1 * ly1;
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            v[e] = (__bf16)(w00 * (float)t00[e] + w01 * (float)t01[e] + w10 * (float)t10[e] + w11 * (float)t11[e]);
                    }
                    seg0 += p.Cf[f];
                }
            }
        }
        bD[ks] = v;
    }

    f32x16 acc2[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[rb][e] = 0.f;
    const int tch = h32_row_channel(l31);         // hidden channel (within a slice) of this lane's row of a transposed box fragment

    // tuning aid: clocks of wave 0 in [0] wait + barrier, [1] nothing (no request ahead: the few clocks between two stamps; tools/head_trace.py keeps the slot), [2] stage 1, [3] gather, [4] ReLU + stage 2, [5] prologue
    // (a clock of the kernel's own, not persist.hpp's PhaseClock: with that hipcc lays the slice loop out differently)
    unsigned long long tsum[6] = {0, 0, 0, 0, 0, 0}, tprev = 0;
    const bool tracing = p.trace != nullptr;
    auto lap = [&](int k) { if (tracing) { const unsigned long long now = __builtin_amdgcn_s_memtime(); tsum[k] += now - tprev; tprev = now; } };
    if (tracing) { tprev = t_begin; lap(5); }
    for (int q = 0; q < p.NQ; ++q) {
        if (q > 0) {
            asm volatile("s_barrier" ::: "memory");
            issue_slice(q);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // my DMA pieces of slice q landed
        asm volatile("s_barrier" ::: "memory");              // everyone's did; everyone is done with slice q-1
        lap(0);
        lap(1);
        const char* const sb = smem;
        // ---- stage 1: 32 hidden channels x 32 pixels; accumulator registers 8 h .. 8 h + 7 = channels 16 h + 8 hi + 0..7, started at
        // the folded-BN shift
        f32x16 acc1 = head_acc_start(sb + OFF_B0, hi);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(sb + OFF_W0 + (ks * 64 + lane) * 16);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bD[ks], acc1, 0, 0, 0);
        }
        lap(2);
        // ---- gather: one more MFMA per wide branch.  A fragment = the box pixels of this slice, transposed on the fly: lane (row l31 ->
        // channel h32_row_channel(l31), k-block hi) reads box pixels 8 hi .. 8 hi + 7 for its channel (eight 2-byte reads, 64-byte stride)
        typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const unsigned short* tp = reinterpret_cast<const unsigned short*>(sb + (wave * 2 + s) * 1024 + (8 * hi) * 64 + tch * 2);
            u16x8 t;
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = tp[e * 32];
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, t), wint[s], acc1, 0, 0, 0);
        }
        lap(3);
        // ---- ReLU -> stage-2 B fragments (a register repack), stage 2: logits += W1[:, q-slice] . h -----------------------------------
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            bf16x8 bH;
#pragma unroll
            for (int e = 0; e < 8; ++e) bH[e] = (__bf16)fmaxf(acc1[8 * h + e], 0.f);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(sb + OFF_W1 + ((rb * 2 + h) * 64 + lane) * 16);
                acc2[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bH, acc2[rb], 0, 0, 0);
            }
        }
        lap(4);
    }
    if (tracing && threadIdx.x == 0 && blockIdx.x % 97 == 0)
        for (int k = 0; k < 6; ++k) p.trace[(size_t)(blockIdx.x / 97) * 8 + k] = tsum[k];
    if constexpr (DEC) {          // log-softmax and the tile's row / column maxima in place of the logits
        static_assert(!DEC || RB == 2, "the two-lane softmax holds 64 channel slots per pixel");
        head_decode_epilogue(p, tl, acc2, smem, wave, hi, l31, valid);
    } else {
        if (valid) head_store_logits32<RB>(p, acc2, pix, hi);
    }
}

// applies when: two gather sources whose per-wave boxes (one output row x 32 columns) hold at most 16 pixels, K1 = ks16 * 16 with an
// instantiated depth, LC a multiple of 8 and at most 64.  Returns false (nothing launched) otherwise: the 16 x 16 x 32 kernel runs.
bool head32_applies(const HeadParams& p) {
    if (!env_int(ENV_HEAD32) || p.nsrc != 2 || !p.w0_32 || !p.w1_32 || p.ks16 != 13 || p.LC > 64 || p.LC % 8) return false;
    return head_boxes_fit(p.sx[0]) && head_boxes_fit(p.sx[1]);
}
void head32_decode_parts(int h, int w, int* row_parts, int* col_parts) { *row_parts = (w + 31) / 32; *col_parts = (h + 3) / 4; }
size_t head32_decode_scratch(int B, int C, int h, int w) {
    int rp, cp;
    head32_decode_parts(h, w, &rp, &cp);
    return ((size_t)B * (C - 1) * h * rp + (size_t)B * cp * (C - 1) * w) * sizeof(float);
}

bool launch_head32(const HeadParams& p, hipStream_t s) {
    if (!head32_applies(p)) return false;
    HeadParams q = p;
    const unsigned blocks = head_set_tiling(q, 32, 4);
    const int rb = (p.LC + 31) / 32;
    TraceScope trace(env_str(ENV_HEAD_TRACE), (size_t)(blocks / 97 + 1) * 8, s);
    q.trace = trace.words;
    const size_t lds = (size_t)(H32_SRC + (13 + rb * 2 + 1) * 1024);
    if (p.dec_row && p.dec_col && rb == 2)       // decode-fused form: 32 KB of LDS for the tile's log-probabilities
        SNCAL_LAUNCH((head32_kernel<2, 13, 1>), dim3(blocks), dim3(256), (size_t)32 * 1024, s, q);
    else if (rb == 2) SNCAL_LAUNCH((head32_kernel<2, 13, 0>), dim3(blocks), dim3(256), lds, s, q);
    else SNCAL_LAUNCH((head32_kernel<1, 13, 0>), dim3(blocks), dim3(256), lds, s, q);
    return true;
}

}  // namespace sncal
