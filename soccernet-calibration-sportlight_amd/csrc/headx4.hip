// Fused HRNet head of the fp16x3 engine at upscale 4 (hrnet_w48x4; the reference's src/models/hrnet/hrnet.py:489-510, :316-329):
// headx3.hip's two GEMMs in split-fp16 arithmetic, for a head at FOUR times branch 0's size.  No tensor sits at head resolution there
// -- the stem (H/2) is interpolated like the branches -- so the stem takes the place of headx3's direct tensor as one more blended
// source:
//
//     stage 1  MFMA x3  h = W0[:, 0:208] . [up(stem) 64 | up(branch 0) 48 | up(branch 1) 96]      (K1 = 13 K-steps of 16, concat order)
//     gather   MFMA x3  h += sum_s t_s . wint_s     t_s = box pixels of W0_s . branch_s (s = 2, 3) at native resolution
//              VALU     h = relu(h)                 (the folded-BN shift is stage 1's initial value), fp32
//     stage 2  MFMA x3  logits += W1[:, 32-slice] . h
// The packed weights are the x2 head's (same columns of last_layer.0, same order).  Branches 0 and 1 and the stem cannot be gathered:
// their boxes for 32 output columns hold more than 16 pixels (head_boxes_fit, head.hpp); blended they cost a tile 13 B fragments once.
// The three source boxes of a tile of 4 rows x 32 columns -- 4 x 18 stem pixels x 64 channels, 3 x 10 x 48, 3 x 6 x 96: 31 KB -- are
// requested once per workgroup as LDS-DMA pieces into the part of LDS that is idle until the top of slice 0 (stage-1 weight buffer 1
// and the stage-2 weight buffers, 35 KB), and every lane blends its pixel's 208 channels out of LDS.  A shape whose boxes do not fit
// there is not served (headx4_fits): the plan then takes the reference formulation.  Slice pipeline, request order and wait counts,
// row order (h32_row_channel), the register repack between the GEMMs and both epilogues (head_frame.hpp) are headx3.hip's.
// Per head pixel the MACs are headx3's (800 x (208 + 32 + 64)); a frame has four times the pixels.
// Compiler's resource report (gfx950): the logits form <0> holds 216 VGPRs, the decode-fused form <1> 225; no spills, scratch 0, no
// static LDS; 79872 B of dynamic LDS per workgroup (X_LDS), two workgroups per CU (headx3: 213 / 222 VGPRs, the same LDS).
#include "persist.hpp"
#include "head.hpp"
#include "softmax_px.hpp"
#include "x3.hpp"

#pragma clang fp contract(off)
#include "head_frame.hpp"

namespace sncal {

typedef x3h8 h16x8;             // (x3.hpp: the 16-bit type of the split)

namespace {
constexpr int KS = 13, RB = 2, NF = HEADX4_FOLD;
constexpr int X_SRC = 16 * 1024;                    // 4 waves x 2 sources x 2 KB (16 box pixels x 32 channels fp32)
constexpr int W0_BUF = 2 * KS * 1024 + 1024;        // [W0 hi 13 KB][W0 lo 13 KB][shift 1 KB], double-buffered
constexpr int OFF_W0 = X_SRC, OFF_W1H = OFF_W0 + 2 * W0_BUF, OFF_W1L = OFF_W1H + RB * 2 * 1024, X_LDS = OFF_W1L + RB * 2 * 1024;      // 79872 B
constexpr int OFF_STAGE = OFF_W0 + W0_BUF, STAGE_BYTES = X_LDS - OFF_STAGE;      // the blended sources' boxes (prologue only): 35840 B
static_assert(2 * X_LDS <= 160 * 1024, "two workgroups per CU");

// worst-case box of a blended source for a tile of 4 rows x 32 columns at scales (sy, sx): rows x columns of source pixels
inline int box_rows(float sy) { return (int)(sy * 3.f) + 3; }
inline int box_cols(float sx) { return (int)(sx * 31.f) + 3; }

__device__ __forceinline__ void split8(const float (&v)[8], h16x8& h, h16x8& l) {
    x3u4 hu, lu;
    x3_split8(v, x3_lower(false), hu, lu);
    h = __builtin_bit_cast(h16x8, hu); l = __builtin_bit_cast(h16x8, lu);
}
__device__ __forceinline__ f32x16 mfma3(const h16x8& ah, const h16x8& al, const h16x8& bh, const h16x8& bl, f32x16 acc) {
    acc = X3_MFMA_32x32x16(al, bh, acc);
    acc = X3_MFMA_32x32x16(ah, bl, acc);
    return X3_MFMA_32x32x16(ah, bh, acc);
}
}  // namespace

template <int DEC>
__global__ __launch_bounds__(256, 2) void headx4_kernel(const HeadX4Params q4) {
    const HeadParams& p = q4.h;
    float amax = 0.f;                                  // range tracker of the hidden vector (x3.hpp; the inputs were tracked by their producers)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HeadTile tl = head_tile(p, 32, 4);
    const int n = tl.n, oy0 = tl.oy0, ox0 = tl.ox0;
    const int y = oy0 + wave, yc = min(y, p.H - 1);
    const int x = ox0 + l31, xc = min(x, p.W - 1);
    const bool valid = y < p.H && x < p.W;
    const long pix = ((long)n * p.H + yc) * p.W + xc;

    // ---- this wave's gather boxes (its row, its 32 columns): two DMA pieces of 64 x 16 B per source and slice, and the bilinear weights
    // of this lane's pixel over the box as a split B fragment
    unsigned dma_voff[2][2];
    h16x8 wih[2], wil[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const HeadBoxTaps b = head_box32<4, 2>(p, s, ox0, yc, xc, lane, dma_voff[s]);
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = head_box_weight(b, 8 * hi + e);
        split8(wv, wih[s], wil[s]);
    }

    const i32x4_t rs_w0h = raw_rsrc(p.w0_32, (unsigned)(p.NQ * KS * 1024)), rs_w0l = raw_rsrc(p.w0_32_lo, (unsigned)(p.NQ * KS * 1024));
    const i32x4_t rs_w1h = raw_rsrc(p.w1_32, (unsigned)(p.NQ * RB * 2 * 1024)), rs_w1l = raw_rsrc(p.w1_32_lo, (unsigned)(p.NQ * RB * 2 * 1024));
    const i32x4_t rs_b0 = raw_rsrc(p.bias0, (unsigned)(p.HP * 4));
    i32x4_t rs_src[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const size_t img = (size_t)p.Hs[s] * p.Ws[s] * p.HP * 4;      // one fp32 image of source s
        rs_src[s] = raw_rsrc(reinterpret_cast<const char*>(p.src[s]) + (size_t)n * img, (unsigned)img);
    }
    const unsigned lds0 = (unsigned)(__UINTPTR_TYPE__)(lds_void*)smem;
    // the three request groups of a slice (headx3.hip).  Boxes: this wave's own region; stage-1 weights + shift: buffer q & 1, requested
    // one slice ahead; stage-2 weights: single-buffered, requested at the top of their slice
    auto issue_boxes = [&](int q) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j) dma_piece(rs_src[s], lds0 + ((wave * 2 + s) * 2 + j) * 1024, dma_voff[s][j], (unsigned)(q * 128));
    };
    auto issue_w0 = [&](int q) {
        const unsigned base = lds0 + OFF_W0 + (q & 1) * W0_BUF;
#pragma unroll
        for (int i = 0; i < (KS + 3) / 4; ++i)
            if (wave + 4 * i < KS) {
                dma_piece(rs_w0h, base + (wave + 4 * i) * 1024, (unsigned)(lane * 16), (unsigned)((q * KS + wave + 4 * i) * 1024));
                dma_piece(rs_w0l, base + KS * 1024 + (wave + 4 * i) * 1024, (unsigned)(lane * 16), (unsigned)((q * KS + wave + 4 * i) * 1024));
            }
        if (wave == 3) dma_piece(rs_b0, base + 2 * KS * 1024, lane < 8 ? (unsigned)(lane * 16) : BUF_OOB, (unsigned)(q * 128));
    };
    auto issue_w1 = [&](int q) {       // RB * 2 = 4 pieces each: one per wave
        dma_piece(rs_w1h, lds0 + OFF_W1H + wave * 1024, (unsigned)(lane * 16), (unsigned)((q * RB * 2 + wave) * 1024));
        dma_piece(rs_w1l, lds0 + OFF_W1L + wave * 1024, (unsigned)(lane * 16), (unsigned)((q * RB * 2 + wave) * 1024));
    };
    issue_boxes(0);
    issue_w0(0);

    // ---- the blended sources' boxes of this tile -> LDS: a box row is contiguous in the source (bw pixels x Cf channels), a box holds at
    // most four rows (launcher), its pieces of 1 KB follow each other from OFF_STAGE on; lanes past the box read zeros
    int f_t0[NF], f_dx[NF], f_dy[NF];       // per source and lane: LDS float index of the lane's first tap, distances to the next column / row
    float f_lx[NF], f_ly[NF];
    {
        int off = 0;
        const int y0c = min(oy0, p.H - 1), y3c = min(oy0 + 3, p.H - 1), x31c = min(ox0 + 31, p.W - 1);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int Hf = q4.Hf[f], Wf = q4.Wf[f], Cf = q4.Cf[f];
            const int iy0 = min((int)(q4.fsy[f] * (float)y0c), Hf - 1), iy3 = min((int)(q4.fsy[f] * (float)y3c), Hf - 1);
            const int ix0 = min((int)(q4.fsx[f] * (float)ox0), Wf - 1), ix1 = min((int)(q4.fsx[f] * (float)x31c), Wf - 1);
            const int nrows = iy3 - iy0 + 1 + (iy3 < Hf - 1 ? 1 : 0), bw = ix1 - ix0 + 1 + (ix1 < Wf - 1 ? 1 : 0);
            const unsigned rowb = (unsigned)(bw * Cf * 4), total = (unsigned)nrows * rowb;
            const int npieces = (int)((total + 1023u) / 1024u);
            const size_t img = (size_t)Hf * Wf * Cf * 4;
            const i32x4_t rs_f = raw_rsrc(reinterpret_cast<const char*>(q4.fold[f]) + (size_t)n * img, (unsigned)img);
            for (int i = wave; i < npieces; i += 4) {
                const unsigned o = (unsigned)((i * 64 + lane) * 16);
                const unsigned row = (o >= rowb ? 1u : 0u) + (o >= 2u * rowb ? 1u : 0u) + (o >= 3u * rowb ? 1u : 0u);
                const unsigned voff = o < total ? (unsigned)(((iy0 + (int)row) * Wf + ix0) * Cf * 4) + (o - row * rowb) : BUF_OOB;
                dma_piece(rs_f, lds0 + OFF_STAGE + (unsigned)(off + i * 1024), voff, 0u);
            }
            const HeadTap tp = head_tap(q4.fsy[f], q4.fsx[f], Hf, Wf, yc, xc);
            f_ly[f] = tp.ly1; f_lx[f] = tp.lx1;
            f_dx[f] = tp.more_x ? Cf : 0;
            f_dy[f] = tp.more_y ? bw * Cf : 0;
            f_t0[f] = (OFF_STAGE + off) / 4 + ((tp.iy - iy0) * bw + (tp.ix - ix0)) * Cf;
            off += npieces * 1024;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");                   // everyone's pieces: the boxes, W0(0), the gather boxes of slice 0

    // ---- stage-1 B fragments, split: lane (pixel l31, k-block hi) holds channels 16 ks + 8 hi .. + 7 of its pixel's blended concat
    // vector.  Segment boundaries (64, 112) are multiples of 8 channels.  torch's bilinear order: blended in x first, then in y
    // (upsample_add's fp32 path, ops.hip)
    auto blend8 = [&](const float* t, int dx, int dy, float lx1, float ly1, float (&v)[8]) __attribute__((always_inline)) {
        const float lx0 = 1.f - lx1, ly0 = 1.f - ly1;
#pragma unroll
        for (int h4 = 0; h4 < 2; ++h4) {
            const float4 t00 = *reinterpret_cast<const float4*>(t + 4 * h4), t01 = *reinterpret_cast<const float4*>(t + dx + 4 * h4);
            const float4 t10 = *reinterpret_cast<const float4*>(t + dy + 4 * h4), t11 = *reinterpret_cast<const float4*>(t + dy + dx + 4 * h4);
            v[4 * h4 + 0] = (t00.x * lx0 + t01.x * lx1) * ly0 + (t10.x * lx0 + t11.x * lx1) * ly1;
            v[4 * h4 + 1] = (t00.y * lx0 + t01.y * lx1) * ly0 + (t10.y * lx0 + t11.y * lx1) * ly1;
            v[4 * h4 + 2] = (t00.z * lx0 + t01.z * lx1) * ly0 + (t10.z * lx0 + t11.z * lx1) * ly1;
            v[4 * h4 + 3] = (t00.w * lx0 + t01.w * lx1) * ly0 + (t10.w * lx0 + t11.w * lx1) * ly1;
        }
    };
    h16x8 bDh[KS], bDl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int kk = ks * 16 + hi * 8;
        float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int seg0 = 0;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (kk >= seg0 && kk < seg0 + q4.Cf[f])
                blend8(reinterpret_cast<const float*>(smem) + f_t0[f] + (kk - seg0), f_dx[f], f_dy[f], f_lx[f], f_ly[f], v);
            seg0 += q4.Cf[f];
        }
        split8(v, bDh[ks], bDl[ks]);
    }

    f32x16 acc2[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc2[rb][e] = 0.f;
    const int tch = h32_row_channel(l31);         // hidden channel (within a slice) of this lane's row of a transposed box fragment

    // Request order per wave from here: per slice q: W1(q), W0(q + 1), boxes(q + 1).  Requests complete in order, so "at most n newest in
    // flight" (vmcnt(n)) names exactly which older groups have landed; a wave issues 6-9 pieces per W0 group (the waits use the smallest
    // count), 2 per W1 group, 4 per box group.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    asm volatile("s_barrier" ::: "memory");                   // everyone has blended: the boxes' LDS goes back to the weights
    for (int q = 0; q < p.NQ; ++q) {
        // here: everyone is done with slice q - 1 and everyone's pieces of W0(q) have landed
        issue_w1(q);                                  // lands under stage 1 + gather
        if (q + 1 < p.NQ) issue_w0(q + 1);            // lands under the whole slice
        const char* const w0b = smem + OFF_W0 + (q & 1) * W0_BUF;
        // ---- stage 1: 32 hidden channels x 32 pixels, started at the folded-BN shift
        f32x16 acc1 = head_acc_start(w0b + 2 * KS * 1024, hi);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const h16x8 ah = *reinterpret_cast<const h16x8*>(w0b + (ks * 64 + lane) * 16);
            const h16x8 al = *reinterpret_cast<const h16x8*>(w0b + KS * 1024 + (ks * 64 + lane) * 16);
            acc1 = mfma3(ah, al, bDh[ks], bDl[ks], acc1);
        }
        // my boxes of slice q (requested after the gather of slice q - 1; newer: W1(q), W0(q + 1)) -- the first slice's landed in the prologue
        if (q > 0) { if (q + 1 < p.NQ) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
        // ---- gather: A fragment = the box pixels of this slice, transposed on the fly and split
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float* tp = reinterpret_cast<const float*>(smem + (wave * 2 + s) * 2048) + (8 * hi) * 32 + tch;
            float tv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) tv[e] = tp[e * 32];
            h16x8 th, tlo;
            split8(tv, th, tlo);
            acc1 = mfma3(th, tlo, wih[s], wil[s], acc1);
        }
        if (q + 1 < p.NQ) {             // my boxes are read: the next slice's travel under stage 2 and stage 1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue_boxes(q + 1);
            asm volatile("s_waitcnt vmcnt(10)" ::: "memory");     // my pieces of W1(q) (newer: W0(q + 1) and the boxes)
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");                   // everyone's pieces of W1(q)
        // ---- ReLU -> split stage-2 B fragments (a register repack), stage 2: logits += W1[:, q-slice] . h
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float hv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = acc1[8 * h + e];
            x3u4 bhu, blu;
            x3_split8(hv, x3_lower(true), bhu, blu, amax);           // ReLU + clamp + split
            const h16x8 bh = __builtin_bit_cast(h16x8, bhu), bl = __builtin_bit_cast(h16x8, blu);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const h16x8 ah = *reinterpret_cast<const h16x8*>(smem + OFF_W1H + ((rb * 2 + h) * 64 + lane) * 16);
                const h16x8 al = *reinterpret_cast<const h16x8*>(smem + OFF_W1L + ((rb * 2 + h) * 64 + lane) * 16);
                acc2[rb] = mfma3(ah, al, bh, bl, acc2[rb]);
            }
        }
        if (q + 1 < p.NQ) {
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // my pieces of W0(q + 1) (newer: the boxes)
            asm volatile("s_barrier" ::: "memory");               // everyone's; and everyone is done with slice q
        }
    }
    x3_report(amax, p.range);
    // decode-fused form (head_frame.hpp): log-softmax and the tile's row / column maxima in place of the logits
    if constexpr (DEC) head_decode_epilogue(p, tl, acc2, smem, wave, hi, l31, valid);
    else if (valid) head_store_logits32<RB>(p, acc2, pix, hi);
}

// The kernel serves: three blended sources of 208 channels together, each a multiple of 8, whose boxes for a tile hold at most four
// rows and fit the idle LDS together; two gathered sources whose per-wave boxes hold at most 16 pixels.
bool headx4_fits(const int* fc, const float* fsy, const float* fsx, const float* gsx) {
    int k = 0, bytes = 0;
    for (int f = 0; f < NF; ++f) {
        if (fc[f] <= 0 || fc[f] % 8 || box_rows(fsy[f]) > 4) return false;
        k += fc[f];
        bytes += (box_rows(fsy[f]) * box_cols(fsx[f]) * fc[f] * 4 + 1023) / 1024 * 1024;
    }
    return k == KS * 16 && bytes <= STAGE_BYTES && head_boxes_fit(gsx[0]) && head_boxes_fit(gsx[1]);
}

// ... and 64 class slots (49..64 classes), the split 32 x 32 x 16 weights, every image a buffer descriptor covers below 2 GB (BUF_OOB)
bool headx4_applies(const HeadX4Params& q) {
    const HeadParams& p = q.h;
    if (p.nsrc != 2 || !p.w0_32 || !p.w0_32_lo || !p.w1_32 || !p.w1_32_lo || p.ks16 != KS || p.LC != 64 || p.HP % 32) return false;
    for (int f = 0; f < NF; ++f)
        if ((size_t)q.Hf[f] * q.Wf[f] * q.Cf[f] * 4 >= (1u << 31)) return false;
    for (int s = 0; s < 2; ++s)
        if ((size_t)p.Hs[s] * p.Ws[s] * p.HP * 4 >= (1u << 31)) return false;
    return headx4_fits(q.Cf, q.fsy, q.fsx, p.sx);
}

bool launch_headx4(const HeadX4Params& p, hipStream_t s) {
    if (!headx4_applies(p)) return false;
    opt_in_lds<&headx4_kernel<0>, &headx4_kernel<1>>(X_LDS);
    HeadX4Params q = p;
    const unsigned blocks = head_set_tiling(q.h, 32, 4);
    if (q.h.dec_row && q.h.dec_col) SNCAL_LAUNCH((headx4_kernel<1>), dim3(blocks), dim3(256), (size_t)X_LDS, s, q);
    else SNCAL_LAUNCH((headx4_kernel<0>), dim3(blocks), dim3(256), (size_t)X_LDS, s, q);
    return true;
}

}  // namespace sncal
