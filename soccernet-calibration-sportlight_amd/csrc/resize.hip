// Frames of any size: cv2.resize(img, (W, H)) with its default INTER_LINEAR on uint8 BGR frames, a batch in one launch.
//   reference: src/models/line/dataset.py:73, baseline/dataloader.py:62, baseline/detect_extremities.py:237
// The arithmetic is OpenCV 4.7's 8-bit path, restated in include/sncal.h; tap() below is its one statement in this file, called on
// the host by sncal_resize_tables and on the device by the kernel, so the tables a test reads are the taps the kernel uses.
// One pass, no intermediate tensor, no workspace: a lane forms the y taps of its row and the x taps of its pixels itself (fp64 for
// the position, as OpenCV; -ffp-contract=off keeps the multiply and the subtraction apart).
// Tiling: one destination pixel per lane in the frame's flat order, in both paths, so that neighbouring lanes read neighbouring
// source bytes.  The byte path stores its three bytes; the wide path (an aligned d_dst and H * W % 16 == 0) gathers a workgroup's
// 256 pixels = 768 B in LDS and 48 lanes store them as 16-byte pieces.  (A first version gave a lane 16 pixels of a row and three
// 16-byte stores, augment.hip's tiling: its gathers were 48 pixels apart from lane to lane and it ran 1.2 - 2.2 x SLOWER than the
// byte path, profiles/resize.md.)  Both call the same pixel functions, so they write the same bits.  Source reads are the same in
// both: the two taps of a row are neighbours
// (x1 == x0 + 1 except at the right clamp), 6 bytes, read as ONE unaligned 8-byte load where 8 bytes lie inside d_src's extent and
// byte by byte at the last pixels of the buffer: the source needs no alignment.  The w == 2 W, h == 2 H area path reads its 2x2 block
// the same way.
#include "common.hpp"
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

constexpr int RS_THREADS = 256;

struct Tap {
    int s, c0, c1;
};

// One destination index of one axis.  `scale` is 1.0 / ((double)n_dst / n_src), formed once on the host.
__host__ __device__ inline Tap tap(int d, double scale, int n_src, bool zero_edges) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (zero_edges) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
    }
    Tap t;
    t.s = s;
    t.c0 = (int)(short)(int)rintf((1.f - f) * 2048.f);
    t.c1 = (int)(short)(int)rintf(f * 2048.f);
    return t;
}

inline double axis_scale(int n_src, int n_dst) { return 1.0 / ((double)n_dst / n_src); }

__host__ __device__ inline int clip(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the pixels at columns x0 and x1 of the row that starts `row` bytes into the source; `limit` = bytes of the whole source
__device__ inline void load_pair(const unsigned char* __restrict__ src, size_t row, size_t limit, int x0, int x1, unsigned p0[3],
                                 unsigned p1[3]) {
    const size_t o0 = row + (unsigned)(x0 * 3);
    if (x1 == x0 + 1 && o0 + 8 <= limit) {
        unsigned long long v;
        __builtin_memcpy(&v, src + o0, 8);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p0[c] = (unsigned)(v >> (8 * c)) & 255u;
            p1[c] = (unsigned)(v >> (8 * (c + 3))) & 255u;
        }
    } else {
        const size_t o1 = row + (unsigned)(x1 * 3);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p0[c] = src[o0 + c];
            p1[c] = src[o1 + c];
        }
    }
}

__device__ inline int mul24(int a, int b) { return __mul24(a, b); }

struct Rows {                             // a destination row's share of the work: two source rows and their weights
    size_t r0, r1;
    int b0, b1;
};

template <bool AREA>
__device__ inline Rows rows_of(int y, size_t frame, int h, int w, double sy) {
    Rows R;
    if (AREA) {
        R.r0 = frame + (unsigned)(2 * y * w * 3);          // inside a frame every offset is below 2^31
        R.r1 = R.r0 + (unsigned)(w * 3);
        R.b0 = R.b1 = 0;
    } else {
        const Tap t = tap(y, sy, h, false);
        R.r0 = frame + (unsigned)(clip(t.s, h - 1) * w * 3);
        R.r1 = frame + (unsigned)(clip(t.s + 1, h - 1) * w * 3);
        R.b0 = t.c0;
        R.b1 = t.c1;
    }
    return R;
}

template <bool AREA>
__device__ inline void pixel(const unsigned char* __restrict__ src, size_t limit, const Rows& R, int x, int w, double sx,
                             unsigned char out[3]) {
    unsigned p00[3], p01[3], p10[3], p11[3];
    if (AREA) {
        load_pair(src, R.r0, limit, 2 * x, 2 * x + 1, p00, p01);
        load_pair(src, R.r1, limit, 2 * x, 2 * x + 1, p10, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (unsigned char)((p00[c] + p01[c] + p10[c] + p11[c] + 2u) >> 2);
    } else {
        const Tap t = tap(x, sx, w, true);
        const int x1 = t.s + 1 < w ? t.s + 1 : w - 1;
        load_pair(src, R.r0, limit, t.s, x1, p00, p01);
        load_pair(src, R.r1, limit, t.s, x1, p10, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // every factor is non-negative and below 2^23 (a byte, a weight in 0..2048, h >> 4 <= 255 * 2049 / 16) and every product is
            // below 2^31: the 24-bit multiplier gives the same integers at four times the rate of the 32-bit one
            const int h0 = (int)(__umul24(p00[c], (unsigned)t.c0) + __umul24(p01[c], (unsigned)t.c1));
            const int h1 = (int)(__umul24(p10[c], (unsigned)t.c0) + __umul24(p11[c], (unsigned)t.c1));
            out[c] = (unsigned char)(((mul24(R.b0, h0 >> 4) >> 16) + (mul24(R.b1, h1 >> 4) >> 16) + 2) >> 2);
        }
    }
}

// ---- wide path: a workgroup's 256 pixels meet in LDS and leave as 48 16-byte stores --------------------------------------------
// A tile is 256 consecutive pixels of the frame's flat order = 768 B, so every tile starts on a 16-byte boundary of an aligned frame,
// and with H * W % 16 == 0 the last, shorter tile is whole 16-byte pieces too.
template <bool AREA>
__global__ __launch_bounds__(RS_THREADS) void resize_wide_kernel(const unsigned char* __restrict__ src, int h, int w,
                                                                 unsigned char* __restrict__ dst, int H, int W, double sx, double sy,
                                                                 size_t limit) {
    __shared__ uint4 tile4[RS_THREADS * 3 / 16];
    unsigned char* tile = reinterpret_cast<unsigned char*>(tile4);
    const int b = blockIdx.y, npix = H * W, t = threadIdx.x;
    const size_t frame = (size_t)b * h * w * 3, n3 = (size_t)npix * 3;
    for (int p0 = blockIdx.x * RS_THREADS; p0 < npix; p0 += gridDim.x * RS_THREADS) {     // uniform over the workgroup: the barriers are met by all
        const int i = p0 + t;
        if (i < npix) {
            const int y = i / W, x = i - y * W;
            const Rows R = rows_of<AREA>(y, frame, h, w, sy);
            unsigned char v[3];
            pixel<AREA>(src, limit, R, x, w, sx, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) tile[3 * t + c] = v[c];
        }
        __syncthreads();
        const int left = npix - p0, pieces = (left < RS_THREADS ? left : RS_THREADS) * 3 / 16;
        if (t < pieces) reinterpret_cast<uint4*>(dst + b * n3 + (size_t)p0 * 3)[t] = tile4[t];
        __syncthreads();
    }
}

// ---- byte path (any W, any alignment): one pixel per lane, byte stores ---------------------------------------------------------
template <bool AREA>
__global__ __launch_bounds__(RS_THREADS) void resize_byte_kernel(const unsigned char* __restrict__ src, int h, int w,
                                                                 unsigned char* __restrict__ dst, int H, int W, double sx, double sy,
                                                                 size_t limit) {
    const int b = blockIdx.y, npix = H * W;
    const size_t frame = (size_t)b * h * w * 3, n3 = (size_t)npix * 3;
    for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < npix; i += gridDim.x * RS_THREADS) {
        const int y = i / W, x = i - y * W;
        const Rows R = rows_of<AREA>(y, frame, h, w, sy);
        unsigned char v[3];
        pixel<AREA>(src, limit, R, x, w, sx, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[b * n3 + (size_t)i * 3 + c] = v[c];
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

template <bool AREA>
void launch(bool wide, dim3 grid, hipStream_t st, const unsigned char* src, int h, int w, unsigned char* dst, int H, int W, double sx,
            double sy, size_t limit) {
    if (wide)
        hipLaunchKernelGGL(resize_wide_kernel<AREA>, grid, dim3(RS_THREADS), 0, st, src, h, w, dst, H, W, sx, sy, limit);
    else
        hipLaunchKernelGGL(resize_byte_kernel<AREA>, grid, dim3(RS_THREADS), 0, st, src, h, w, dst, H, W, sx, sy, limit);
}

}  // namespace

extern "C" int sncal_resize_tables(int n_src, int n_dst, int zero_edges, int32_t* ofs, int16_t* coef) {
    SNCAL_CHECK_ARG(n_src >= 1 && n_dst >= 1, "sncal_resize_tables: n_src=%d n_dst=%d (both >= 1)", n_src, n_dst);
    SNCAL_CHECK_ARG(ofs && coef, "sncal_resize_tables: null pointer");
    const double scale = axis_scale(n_src, n_dst);
    for (int d = 0; d < n_dst; ++d) {
        const Tap t = tap(d, scale, n_src, zero_edges != 0);
        ofs[d] = t.s;
        coef[2 * d] = (int16_t)t.c0;
        coef[2 * d + 1] = (int16_t)t.c1;
    }
    return SNCAL_OK;
}

extern "C" int sncal_resize_u8(const unsigned char* d_src, int B, int h, int w, unsigned char* d_dst, int H, int W, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && B <= 65535 && h >= 1 && w >= 1 && H >= 1 && W >= 1,
                    "sncal_resize_u8: B=%d h=%d w=%d H=%d W=%d (B <= 65535, every dimension >= 1)", B, h, w, H, W);
    SNCAL_CHECK_ARG((long long)h * w * 3 < (1ll << 31) && (long long)H * W * 3 < (1ll << 31),
                    "sncal_resize_u8: a frame of %d x %d x 3 or %d x %d x 3 elements is past 2^31", h, w, H, W);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_src && d_dst, "sncal_resize_u8: null pointer");
    const size_t n_src = (size_t)B * h * w * 3, n_dst = (size_t)B * H * W * 3;
    SNCAL_CHECK_ARG(!overlap(d_src, n_src, d_dst, n_dst), "sncal_resize_u8: d_src overlaps d_dst");
    hipStream_t st = sncal::as_stream(stream);
    if (h == H && w == W) {                                 // OpenCV copies too
        SNCAL_CHECK_HIP(hipMemcpyAsync(d_dst, d_src, n_dst, hipMemcpyDeviceToDevice, st));
        return SNCAL_OK;
    }
    const bool wide = (long long)H * W % 16 == 0 && ((uintptr_t)d_dst & 15) == 0;
    long long blocks = ((long long)H * W + RS_THREADS - 1) / RS_THREADS;
    const long long cap = 2048 / B > 0 ? 2048 / B : 1;      // about eight workgroups per compute unit over the batch; the rest by grid stride
    if (blocks > cap) blocks = cap;
    const dim3 grid((unsigned)blocks, B);
    const double sx = axis_scale(w, W), sy = axis_scale(h, H);
    if (w == 2 * W && h == 2 * H)
        launch<true>(wide, grid, st, d_src, h, w, d_dst, H, W, sx, sy, n_src);
    else
        launch<false>(wide, grid, st, d_src, h, w, d_dst, H, W, sx, sy, n_src);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
