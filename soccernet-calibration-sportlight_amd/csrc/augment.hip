// Train-time image augmentation, fused: ColorAugment -> GaussNoise -> Flip -> (uint8 BGR and / or ToTensor's fp32 CHW)
//   /root/reference/src/models/hrnet/transforms.py:16-68, 122-133 (the line model's copies: src/models/line/transforms.py:10-139)
// Two kernels, no atomics:
//   1. augment_sums_kernel   per frame with the colour flag: the EXACT integer sum of each channel.  A workgroup writes its three
//      64-bit partials into the workspace; workgroups of a frame without the flag exit at once.
//   2. augment_apply_kernel  folds a frame's partials in index order (integers: the order cannot matter, it is fixed anyway), forms
//      mean[c] = double(S_c) * gain[c] / double(H*W), then reads every source element once and writes each output once:
//        colour  p = double(x) * gain[c];  v = (p - mean[c]) * contrast + mean[c];  clip to [0, 255];  truncate       (fp64, no contraction)
//        noise   v = double(u8) + d_noise[e], clip, truncate (fp64)      when the caller hands the normals in
//                v = float(u8) + float(noise_sigma) * z, clip, truncate  (fp32) with z from Philox4x32-10 + Box-Muller otherwise
//        flip    out[b, y, W-1-x, :] = v[b, y, x, :]
//      The uint8 truncation between the stages is the reference's.
// Device noise: the Philox key is the frame's seed, the counter the index of the element quad in the frame's flat SOURCE order
// (element e = (y*W + x)*3 + c, quad e / 4); one counter gives four uniforms, Box-Muller turns (u0, u1) and (u2, u3) into four
// normals, element e takes normal e % 4.  Nothing else enters: not the batch index, not the tiling, not the flip.
// Tiling: a lane of the wide path owns 16 pixels of a row = 48 B = three 16-byte loads; its mirrored store covers the 16 pixels
// [W-16-x0, W-x0), again 16-byte aligned when W % 16 == 0 and the bases are.  Every other shape or alignment takes the narrow path,
// one pixel per lane with byte accesses; both paths call the same per-element functions, so they write the same bits.
#include "common.hpp"
#include <cstdint>

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_SUM_BLOCKS = 64;        // most partials a frame can have
constexpr int AUG_UNIT = 16;              // pixels per lane on the wide path
constexpr unsigned FLAG_COLOUR = 1u, FLAG_NOISE = 2u, FLAG_FLIP = 4u;

__host__ __device__ inline int sum_blocks(long long n3) {
    const long long per = (long long)AUG_THREADS * AUG_UNIT * 3;
    const long long k = (n3 + per - 1) / per;
    return (int)(k < 1 ? 1 : (k > AUG_SUM_BLOCKS ? AUG_SUM_BLOCKS : k));
}

// ---- channel sums --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void augment_sums_kernel(const unsigned char* __restrict__ src, int n3,
                                                                   const sncal_augment_params* __restrict__ params,
                                                                   unsigned long long* __restrict__ part) {
    const int b = blockIdx.y, k = blockIdx.x, nblk = gridDim.x, t = threadIdx.x;
    if (!(params[b].flags & FLAG_COLOUR)) return;
    const unsigned char* f = src + (size_t)b * n3;
    unsigned s[3] = {0u, 0u, 0u};                            // a lane sees at most n3 / 256 bytes: < 2^31 in all
    if (((uintptr_t)f & 15) == 0) {
        const int units = n3 / 48;
        for (int u = k * AUG_THREADS + t; u < units; u += nblk * AUG_THREADS) {
            const uint4* p = reinterpret_cast<const uint4*>(f + (size_t)u * 48);
            const uint4 q[3] = {p[0], p[1], p[2]};
            const unsigned w[12] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
#pragma unroll
            for (int j = 0; j < 48; ++j) s[j % 3] += (w[j >> 2] >> ((j & 3) * 8)) & 255u;
        }
        if (k == nblk - 1)
            for (int i = units * 48 + t; i < n3; i += AUG_THREADS) s[i % 3] += f[i];
    } else {
        const int npix = n3 / 3;
        for (int i = k * AUG_THREADS + t; i < npix; i += nblk * AUG_THREADS) {
            s[0] += f[(size_t)i * 3];
            s[1] += f[(size_t)i * 3 + 1];
            s[2] += f[(size_t)i * 3 + 2];
        }
    }
    __shared__ unsigned long long sh[AUG_THREADS / 64][3];
    unsigned long long v[3] = {s[0], s[1], s[2]};
#pragma unroll
    for (int c = 0; c < 3; ++c)
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_down(v[c], o, 64);
    if ((t & 63) == 0)
        for (int c = 0; c < 3; ++c) sh[t >> 6][c] = v[c];
    __syncthreads();
    if (t < 3) {
        unsigned long long a = 0;
        for (int w = 0; w < AUG_THREADS / 64; ++w) a += sh[w][t];
        part[((size_t)b * nblk + k) * 3 + t] = a;
    }
}

// ---- per-element arithmetic, shared by the wide and the narrow path ----------------------------------------------------
struct Frame {
    double gain[3], mean[3], contrast;
    float sigma;
    unsigned k0, k1, flags;
};

__device__ inline unsigned char colour1(unsigned x, int c, const Frame& F) {
    const double p = (double)x * F.gain[c];
    double v = (p - F.mean[c]) * F.contrast + F.mean[c];
    v = fmin(fmax(v, 0.0), 255.0);
    return (unsigned char)(int)v;
}

__device__ inline unsigned char noise1_f64(unsigned x, double n) {
    double v = (double)x + n;
    v = fmin(fmax(v, 0.0), 255.0);
    return (unsigned char)(int)v;
}

__device__ inline unsigned char noise1_f32(unsigned x, float z, float sigma) {
    float v = (float)x + sigma * z;
    v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (unsigned char)(int)v;
}

// Philox4x32-10 (Salmon et al., SC'11), counter (q, 0, 0, 0), key (k0, k1)
__device__ inline void philox(unsigned q, unsigned k0, unsigned k1, unsigned r[4]) {
    unsigned c0 = q, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// four standard normals of quad q: Box-Muller in fp32 on (u0, u1) and (u2, u3); u in (0, 1] for the logarithm, the angle in
// revolutions [0, 1) for the hardware sine / cosine (which take revolutions)
__device__ inline void normal_quad(unsigned q, unsigned k0, unsigned k1, float z[4]) {
    unsigned r[4];
    philox(q, k0, k1, r);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float u = (float)((r[2 * i] >> 8) + 1u) * 0x1p-24f;
        const float a = (float)(r[2 * i + 1] >> 8) * 0x1p-24f;
        const float rad = __fsqrt_rn(-1.3862943611198906f * __log2f(u));          // -2 ln u = -2 ln 2 * log2 u
        z[2 * i] = rad * __builtin_amdgcn_cosf(a);
        z[2 * i + 1] = rad * __builtin_amdgcn_sinf(a);
    }
}

__device__ inline void load_frame(Frame& F, const sncal_augment_params* __restrict__ params, const unsigned long long* __restrict__ part,
                                  int b, int nsum, int npix) {
    const sncal_augment_params P = params[b];
    F.flags = P.flags;
    F.contrast = P.contrast;
    F.sigma = (float)P.noise_sigma;
    F.k0 = (unsigned)(P.seed & 0xffffffffull);
    F.k1 = (unsigned)(P.seed >> 32);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        F.gain[c] = P.gain[c];
        F.mean[c] = 0.0;
    }
    if (P.flags & FLAG_COLOUR) {
        unsigned long long S[3] = {0ull, 0ull, 0ull};
        for (int k = 0; k < nsum; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) S[c] += part[((size_t)b * nsum + k) * 3 + c];
#pragma unroll
        for (int c = 0; c < 3; ++c) F.mean[c] = (double)S[c] * P.gain[c] / (double)npix;
    }
}

// ---- apply: wide path ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void augment_apply_wide_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                                         const sncal_augment_params* __restrict__ params,
                                                                         const unsigned long long* __restrict__ part, int nsum,
                                                                         const double* __restrict__ noise, unsigned char* __restrict__ dst,
                                                                         float* __restrict__ chw) {
    const int b = blockIdx.y, npix = H * W, units = npix / AUG_UNIT;
    Frame F;
    load_frame(F, params, part, b, nsum, npix);            // uniform over the workgroup: scalar loads, registers
    const size_t n3 = (size_t)npix * 3;
    const bool flip = F.flags & FLAG_FLIP;
    for (int u = blockIdx.x * AUG_THREADS + threadIdx.x; u < units; u += gridDim.x * AUG_THREADS) {
        const size_t e0 = (size_t)u * 48;                  // first element of the unit in the frame's flat source order
        const uint4* p = reinterpret_cast<const uint4*>(src + b * n3 + e0);
        const uint4 q[3] = {p[0], p[1], p[2]};
        const unsigned w[12] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x, q[2].y, q[2].z, q[2].w};
        unsigned char v[48];
#pragma unroll
        for (int j = 0; j < 48; ++j) v[j] = (unsigned char)((w[j >> 2] >> ((j & 3) * 8)) & 255u);
        if (F.flags & FLAG_COLOUR) {
#pragma unroll
            for (int j = 0; j < 48; ++j) v[j] = colour1(v[j], j % 3, F);
        }
        if (F.flags & FLAG_NOISE) {
            if (noise) {
                const double2* n2 = reinterpret_cast<const double2*>(noise + b * n3 + e0);
#pragma unroll
                for (int j = 0; j < 24; ++j) {
                    const double2 n = n2[j];
                    v[2 * j] = noise1_f64(v[2 * j], n.x);
                    v[2 * j + 1] = noise1_f64(v[2 * j + 1], n.y);
                }
            } else {
#pragma unroll
                for (int g = 0; g < 12; ++g) {
                    float z[4];
                    normal_quad((unsigned)(e0 / 4) + g, F.k0, F.k1, z);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[4 * g + i] = noise1_f32(v[4 * g + i], z[i], F.sigma);
                }
            }
        }
        const int pix0 = u * AUG_UNIT, y = pix0 / W, x0 = pix0 - y * W;
        int xd = x0;
        if (flip) {                                        // reverse the 16 pixels, keep each pixel's channel order
            xd = W - AUG_UNIT - x0;
#pragma unroll
            for (int i = 0; i < AUG_UNIT / 2; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned char a = v[3 * i + c];
                    v[3 * i + c] = v[3 * (AUG_UNIT - 1 - i) + c];
                    v[3 * (AUG_UNIT - 1 - i) + c] = a;
                }
        }
        const size_t pd = (size_t)y * W + xd;              // first destination pixel
        if (dst) {
            unsigned o[12];
#pragma unroll
            for (int j = 0; j < 12; ++j)
                o[j] = (unsigned)v[4 * j] | ((unsigned)v[4 * j + 1] << 8) | ((unsigned)v[4 * j + 2] << 16) | ((unsigned)v[4 * j + 3] << 24);
            uint4* d = reinterpret_cast<uint4*>(dst + b * n3 + pd * 3);
            d[0] = make_uint4(o[0], o[1], o[2], o[3]);
            d[1] = make_uint4(o[4], o[5], o[6], o[7]);
            d[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
        if (chw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float4* d = reinterpret_cast<float4*>(chw + ((size_t)b * 3 + c) * npix + pd);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    d[i] = make_float4((float)v[3 * (4 * i) + c] / 255.0f, (float)v[3 * (4 * i + 1) + c] / 255.0f,
                                       (float)v[3 * (4 * i + 2) + c] / 255.0f, (float)v[3 * (4 * i + 3) + c] / 255.0f);
            }
        }
    }
}

// ---- apply: narrow path (any W, any alignment): one pixel per lane, byte accesses ---------------------------------------
__global__ __launch_bounds__(AUG_THREADS) void augment_apply_narrow_kernel(const unsigned char* __restrict__ src, int H, int W,
                                                                           const sncal_augment_params* __restrict__ params,
                                                                           const unsigned long long* __restrict__ part, int nsum,
                                                                           const double* __restrict__ noise, unsigned char* __restrict__ dst,
                                                                           float* __restrict__ chw) {
    const int b = blockIdx.y, npix = H * W;
    Frame F;
    load_frame(F, params, part, b, nsum, npix);
    const size_t n3 = (size_t)npix * 3;
    const bool flip = F.flags & FLAG_FLIP;
    for (int i = blockIdx.x * AUG_THREADS + threadIdx.x; i < npix; i += gridDim.x * AUG_THREADS) {
        const size_t e0 = (size_t)i * 3;
        unsigned char v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = src[b * n3 + e0 + c];
        if (F.flags & FLAG_COLOUR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = colour1(v[c], c, F);
        }
        if (F.flags & FLAG_NOISE) {
            if (noise) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = noise1_f64(v[c], noise[b * n3 + e0 + c]);
            } else {
                const unsigned q0 = (unsigned)(e0 / 4), q1 = (unsigned)((e0 + 2) / 4);       // a pixel's three elements meet at most two quads
                float za[4], zb[4];
                normal_quad(q0, F.k0, F.k1, za);
                normal_quad(q1, F.k0, F.k1, zb);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned e = (unsigned)(e0 + c);
                    const bool first = e / 4 == q0;
                    const int s = e & 3;
                    const float z0 = first ? za[0] : zb[0], z1 = first ? za[1] : zb[1], z2 = first ? za[2] : zb[2], z3 = first ? za[3] : zb[3];
                    const float z = s == 0 ? z0 : s == 1 ? z1 : s == 2 ? z2 : z3;
                    v[c] = noise1_f32(v[c], z, F.sigma);
                }
            }
        }
        const int y = i / W, x = i - y * W;
        const size_t pd = (size_t)y * W + (flip ? W - 1 - x : x);
        if (dst) {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[b * n3 + pd * 3 + c] = v[c];
        }
        if (chw) {
#pragma unroll
            for (int c = 0; c < 3; ++c) chw[((size_t)b * 3 + c) * npix + pd] = (float)v[c] / 255.0f;
        }
    }
}

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int check_shape(const char* who, int B, int H, int W) {
    SNCAL_CHECK_ARG(B >= 0 && B <= 65535 && H >= 1 && W >= 1, "%s: B=%d H=%d W=%d (B <= 65535, H, W >= 1)", who, B, H, W);
    SNCAL_CHECK_ARG((long long)H * W * 3 < (1ll << 31), "%s: a frame of %d x %d x 3 elements is past 2^31", who, H, W);
    return SNCAL_OK;
}

size_t ws_need(int B, int H, int W) {
    const size_t n = (size_t)B * sum_blocks((long long)H * W * 3) * 3 * sizeof(unsigned long long);
    return (n + 15) & ~(size_t)15;
}

}  // namespace

extern "C" int sncal_augment_workspace(int B, int H, int W, size_t* bytes) {
    SNCAL_CHECK_ARG(bytes, "sncal_augment_workspace: null pointer");
    if (int st = check_shape("sncal_augment_workspace", B, H, W)) return st;
    *bytes = ws_need(B, H, W);
    return SNCAL_OK;
}

extern "C" int sncal_augment_u8(const unsigned char* d_src, int B, int H, int W, const sncal_augment_params* d_params,
                                const double* d_noise, unsigned char* d_dst, float* d_chw, void* d_ws, size_t ws_bytes, void* stream) {
    if (int st = check_shape("sncal_augment_u8", B, H, W)) return st;
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_src && d_params, "sncal_augment_u8: null pointer");
    SNCAL_CHECK_ARG(d_dst || d_chw, "sncal_augment_u8: both outputs are null");
    const size_t n3 = (size_t)H * W * 3, n = (size_t)B * n3;
    SNCAL_CHECK_ARG(!(d_dst && overlap(d_src, n, d_dst, n)) && !(d_chw && overlap(d_src, n, d_chw, n * sizeof(float))),
                    "sncal_augment_u8: d_src overlaps an output (the flip reads and writes different columns)");
    SNCAL_CHECK_ARG(!(d_dst && d_chw && overlap(d_dst, n, d_chw, n * sizeof(float))), "sncal_augment_u8: the two outputs overlap");
    SNCAL_CHECK_ARG(!(d_noise && ((d_dst && overlap(d_noise, n * sizeof(double), d_dst, n)) ||
                                  (d_chw && overlap(d_noise, n * sizeof(double), d_chw, n * sizeof(float))))),
                    "sncal_augment_u8: d_noise overlaps an output");
    SNCAL_CHECK_ARG(d_ws && ((uintptr_t)d_ws & 15) == 0, "sncal_augment_u8: workspace pointer null or not 16-byte aligned");
    const size_t need = ws_need(B, H, W);
    if (ws_bytes < need) {
        sncal::set_error("sncal_augment_u8: workspace %zu bytes, need %zu (sncal_augment_workspace)", ws_bytes, need);
        return SNCAL_ERR_WORKSPACE;
    }
    hipStream_t st = sncal::as_stream(stream);
    unsigned long long* part = static_cast<unsigned long long*>(d_ws);
    const int nsum = sum_blocks((long long)n3);
    hipLaunchKernelGGL(augment_sums_kernel, dim3(nsum, B), dim3(AUG_THREADS), 0, st, d_src, (int)n3, d_params, part);
    SNCAL_CHECK_LAUNCH();
    const bool wide = W % AUG_UNIT == 0 && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0 && ((uintptr_t)d_chw & 15) == 0 &&
                      ((uintptr_t)d_noise & 15) == 0;
    const long long work = wide ? (long long)H * W / AUG_UNIT : (long long)H * W;
    long long blocks = (work + AUG_THREADS - 1) / AUG_THREADS;
    const long long cap = 2048 / B > 0 ? 2048 / B : 1;      // about eight workgroups per compute unit over the batch; the rest by grid stride
    if (blocks > cap) blocks = cap;
    if (wide)
        hipLaunchKernelGGL(augment_apply_wide_kernel, dim3((unsigned)blocks, B), dim3(AUG_THREADS), 0, st, d_src, H, W, d_params, part, nsum,
                           d_noise, d_dst, d_chw);
    else
        hipLaunchKernelGGL(augment_apply_narrow_kernel, dim3((unsigned)blocks, B), dim3(AUG_THREADS), 0, st, d_src, H, W, d_params, part, nsum,
                           d_noise, d_dst, d_chw);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
