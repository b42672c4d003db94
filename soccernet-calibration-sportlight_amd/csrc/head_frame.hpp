// Device pieces shared by the three fused-head kernels (head.hip 16 x 16 x 32 bf16, head32.hip 32 x 32 x 16 bf16, headx3.hip split-fp16):
// tile decode, the align_corners=True tap, and for the two 32-wide kernels the per-wave gather box, the accumulator start, the
// decode-fused epilogue and the logits store.  Include it AFTER the includer's `#pragma clang fp contract`: the functions here take the
// includer's contraction mode (fast in head.hip / head32.hip, off in headx3.hip).  The includer includes softmax_px.hpp itself, IN
// FRONT of that pragma (the epilogue below calls it): the per-pixel softmax must stay uncontracted to match the softmax kernels bit
// for bit, so this header deliberately does not include it.
#pragma once
#include "head.hpp"
#include "persist.hpp"

namespace sncal {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) void lds_void;

// which tile of which frame this workgroup owns: multiply-high by host reciprocals (head_set_tiling) instead of emulated integer
// divisions (~25 VALU instructions each)
struct HeadTile { int n, ty, tx, oy0, ox0; };
__device__ __forceinline__ HeadTile head_tile(const HeadParams& p, int tile_w, int tile_h) {
    const int tile = blockIdx.x;
    const unsigned q1 = p.tiles_x == 1 ? (unsigned)tile : __umulhi((unsigned)tile, p.tiles_x_magic);
    const int tx = tile - (int)q1 * p.tiles_x;
    const unsigned q2 = p.tiles_y == 1 ? q1 : __umulhi(q1, p.tiles_y_magic);
    const int ty = (int)q1 - (int)q2 * p.tiles_y;
    return {(int)q2, ty, tx, ty * tile_h, tx * tile_w};
}

// PyTorch's align_corners=True source index of output pixel (yc, xc) in an Hs x Ws map at scales (sy, sx): the clamped top-left tap,
// the fractions towards the next row / column, and whether that row / column exists.  head_tap_axis is one axis of it (the gather box
// takes its row before and its column after the box geometry).
struct HeadTapAxis { int i; float l1; bool more; };
__device__ __forceinline__ HeadTapAxis head_tap_axis(float scale, int size, int c) {
    const float f = scale * (float)c;
    int i = (int)f;
    i = i > size - 1 ? size - 1 : i;
    return {i, f - (float)i, i < size - 1};
}
struct HeadTap { int iy, ix; float ly1, lx1; bool more_y, more_x; };
__device__ __forceinline__ HeadTap head_tap(float sy, float sx, int Hs, int Ws, int yc, int xc) {
    const HeadTapAxis y = head_tap_axis(sy, Hs, yc), x = head_tap_axis(sx, Ws, xc);
    return {y.i, x.i, y.l1, x.l1, y.more, x.more};
}

// ---- 32-wide kernels: a wave owns 32 pixels of one output row ---------------------------------------------------------------------
// Source box of gather source s for that row and its 32 columns (<= 16 pixels: head_boxes_fit on the host): the per-lane byte offsets
// of its DMA pieces of 64 x 16 B -- ESZ = element bytes of the source (2 / 4), NPIECE = 32 * ESZ / 64 pieces per source and slice --
// and this lane's four taps as (slot in the box, bilinear weight)
struct HeadBoxTaps { int t00, t01, t10, t11; float w00, w01, w10, w11; };
template <int ESZ, int NPIECE>
__device__ __forceinline__ HeadBoxTaps head_box32(const HeadParams& p, int s, int ox0, int yc, int xc, int lane, unsigned (&dma_voff)[NPIECE]) {
    const int xlast = min(ox0 + 31, p.W - 1);
    const HeadTapAxis ty = head_tap_axis(p.sy[s], p.Hs[s], yc);
    const int by0 = ty.i, nrows = ty.more ? 2 : 1;
    const int bx0 = (int)(p.sx[s] * (float)ox0);
    const int bx1 = min((int)(p.sx[s] * (float)xlast) + 1, p.Ws[s] - 1);
    const int bw = bx1 - bx0 + 1, npx = nrows * bw;
#pragma unroll
    for (int j = 0; j < NPIECE; ++j) {
        const int slot = j * 64 + lane, pi = slot >> (ESZ == 2 ? 2 : 3), part = slot & (2 * ESZ - 1);      // 2 * ESZ lanes of 16 B per box pixel
        const int ly = pi >= bw ? 1 : 0, lx = pi - ly * bw;
        dma_voff[j] = pi < npx ? (unsigned)((((by0 + ly) * p.Ws[s] + bx0 + lx) * p.HP) * ESZ + part * 16) : BUF_OOB;
    }
    const HeadTapAxis tx = head_tap_axis(p.sx[s], p.Ws[s], xc);
    const float ly1 = ty.l1, lx1 = tx.l1;
    const float w00 = (1.f - lx1) * (1.f - ly1), w01 = lx1 * (1.f - ly1), w10 = (1.f - lx1) * ly1, w11 = lx1 * ly1;
    const int t00 = tx.i - bx0, t01 = t00 + (tx.more ? 1 : 0), t10 = t00 + (nrows == 2 ? bw : 0), t11 = t10 + (tx.more ? 1 : 0);
    return {t00, t01, t10, t11, w00, w01, w10, w11};
}
// B fragment of the interpolation GEMM: lane (pixel l31, k-block hi) holds the weights of box pixels 8 hi .. 8 hi + 7; this is the
// weight of box pixel `slot` -- zero where it is not one of the lane's four taps
__device__ __forceinline__ float head_box_weight(const HeadBoxTaps& b, int slot) {
    float w = 0.f;
    w += slot == b.t00 ? b.w00 : 0.f;
    w += slot == b.t01 ? b.w01 : 0.f;
    w += slot == b.t10 ? b.w10 : 0.f;
    w += slot == b.t11 ? b.w11 : 0.f;
    return w;
}

// stage 1 starts at the folded-BN shift of the slice (32 floats in LDS): accumulator registers 8 h .. 8 h + 7 = channels 16 h + 8 hi + 0..7
__device__ __forceinline__ f32x16 head_acc_start(const char* shift, int hi) {
    f32x16 acc1;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float4 b0 = *reinterpret_cast<const float4*>(shift + (16 * h + 8 * hi) * 4);
        const float4 b1 = *reinterpret_cast<const float4*>(shift + (16 * h + 8 * hi + 4) * 4);
        acc1[8 * h + 0] = b0.x; acc1[8 * h + 1] = b0.y; acc1[8 * h + 2] = b0.z; acc1[8 * h + 3] = b0.w;
        acc1[8 * h + 4] = b1.x; acc1[8 * h + 5] = b1.y; acc1[8 * h + 6] = b1.z; acc1[8 * h + 7] = b1.w;
    }
    return acc1;
}

// Decode-fused epilogue (64 class slots: two 32-row blocks): log-softmax per pixel (softmax_px.hpp: bit-identical to the softmax
// kernels), then the tile's maxima per class -- over its 32 columns for every row, over its 4 rows for every column -- which is all the
// keypoint decode needs (transforms.py:230-238: argmax of the column maxima / row maxima).  The (N,58,h,w) log-probabilities and the
// logits are never written: 2 x 2.1 GB per 64 frames less HBM traffic and one kernel less.
__device__ __forceinline__ void head_decode_epilogue(const HeadParams& p, const HeadTile& tl, const f32x16 (&acc2)[2], char* smem,
                                                     int wave, int hi, int l31, bool valid) {
    float v[32], r[32];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = rb * 32 + 16 * h + 8 * hi;
            const float4 b0 = *reinterpret_cast<const float4*>(p.bias1 + c), b1 = *reinterpret_cast<const float4*>(p.bias1 + c + 4);
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * (2 * rb + h) + e] = c + e < p.dec_C ? acc2[rb][8 * h + e] + bb[e] : -INFINITY;
        }
    logsoftmax_px32x2(v, hi, p.dec_C, r);
    // [row of the tile][class][pixel] in LDS (the slice buffers are free: everyone is past the last slice)
    asm volatile("s_barrier" ::: "memory");
    float* const s_lp = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) s_lp[(wave * 64 + 16 * k + 8 * hi + e) * 32 + l31] = valid ? r[8 * k + e] : -INFINITY;
    __syncthreads();
    const int C1 = p.dec_C - 1, t = threadIdx.x;
    {   // row maxima: thread -> (row t >> 6, class t & 63)
        const int rw = t >> 6, c = t & 63, yy = tl.oy0 + rw;
        if (c < C1 && yy < p.H) {
            const float4* q = reinterpret_cast<const float4*>(s_lp + (rw * 64 + c) * 32);
            float m = -INFINITY;
#pragma unroll
            for (int i = 0; i < 8; ++i) { const float4 u = q[i]; m = fmaxf(m, fmaxf(fmaxf(u.x, u.y), fmaxf(u.z, u.w))); }
            p.dec_row[(((size_t)tl.n * C1 + c) * p.H + yy) * p.tiles_x + tl.tx] = m;
        }
    }
    for (int id = t; id < C1 * 32; id += 256) {      // column maxima: (class id >> 5, column id & 31)
        const int c = id >> 5, xx = id & 31;
        if (tl.ox0 + xx < p.W) {
            const float m = fmaxf(fmaxf(s_lp[(0 * 64 + c) * 32 + xx], s_lp[(1 * 64 + c) * 32 + xx]), fmaxf(s_lp[(2 * 64 + c) * 32 + xx], s_lp[(3 * 64 + c) * 32 + xx]));
            p.dec_col[(((size_t)tl.n * p.tiles_y + tl.ty) * C1 + c) * p.W + tl.ox0 + xx] = m;
        }
    }
}

// logits (+ conv bias) -> fp32 NHWC [P][LC]; registers 8 h .. 8 h + 7 of block rb = classes 32 rb + 16 h + 8 hi + 0..7 of pixel `pix`
template <int RB>
__device__ __forceinline__ void head_store_logits32(const HeadParams& p, const f32x16 (&acc2)[RB], long pix, int hi) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = rb * 32 + 16 * h + 8 * hi;
            if (c < p.LC) {
                const float4 b0 = *reinterpret_cast<const float4*>(p.bias1 + c), b1 = *reinterpret_cast<const float4*>(p.bias1 + c + 4);
                float* o = p.logits + pix * p.LC + c;
                *reinterpret_cast<float4*>(o) = make_float4(acc2[rb][8 * h] + b0.x, acc2[rb][8 * h + 1] + b0.y, acc2[rb][8 * h + 2] + b0.z, acc2[rb][8 * h + 3] + b0.w);
                *reinterpret_cast<float4*>(o + 4) = make_float4(acc2[rb][8 * h + 4] + b1.x, acc2[rb][8 * h + 5] + b1.y, acc2[rb][8 * h + 6] + b1.z, acc2[rb][8 * h + 7] + b1.w);
            }
        }
}

}  // namespace sncal
