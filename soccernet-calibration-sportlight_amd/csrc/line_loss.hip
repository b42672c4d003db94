// The loss and validation tail of the line model: the two-peak target maps, EHMLoss.forward for num_refinement_stages = 0 in ONE
// read of the softmax heatmap, its gradient in one more read and one write, and the tp / fp / fn counts of AccMetric
//   /root/reference/src/models/line/dataset.py:107-178 (_generate_keypoint_maps, _add_gaussian)
//   /root/reference/src/models/line/loss.py:34-108     (forward, gmse_loss, adaptive_wing)
//   /root/reference/src/models/line/metrics.py:53-103  (a_t_score)
// Target: a channel holds up to two Gaussians, centred on mu = (min(w-1, rint(x/stride)), min(h-1, rint(y/stride))) (fp32
// division, ties to even, no lower clamp) and divided by their maximum over the grid.  Both are separable, and so is the maximum
// (1 unless mu < 0, then the value at index 0), so one factor is
//     g[i] = exp(-((i - mu)^2 - min(mu, 0)^2) / (2 sigma^2)),     evaluated in fp64 and rounded once (line_gauss1)
// and an element is gx0[x]*gy0[y] + gx1[x]*gy1[y] in fp32, first point first (line_target_value).  A point whose flag is not 1
// has all-zero factors.
//   sncal_line_target   a thread owns one column of a 32-row strip of one channel: its two column factors in registers, the
//                       strip's row factors in LDS; 2*(w + 32) exps per 32*w stores
//   sncal_line_loss     line_tables_kernel writes the factors of every (frame, channel) to the workspace once; line_loss_kernel
//                       has the tiling of loss.hip's loss_kernel (4 waves x LS_R rows x 64*V columns, V = 4 with 16-byte loads
//                       when w % 4 == 0 and the bases are aligned, else 1), walks the C channels, sums a channel's LS_R*V
//                       elements in fp32, folds into two fp64 accumulators per lane; wave shuffle -> LDS -> one partial per
//                       workgroup; line_fold_kernel adds the partials of a frame in index order.  No atomics: two runs give the
//                       same bits.  REBUILD = false reads the target from memory instead (maps as a loader delivers them); fed
//                       with sncal_line_target's output it sees the very values REBUILD = true forms, in the same order.
//   sncal_ehm_loss_grad    the gradient of that loss with respect to the prediction (torch autograd through line/loss.py:61-108,
//                       the target held fixed): line_grad_kernel is line_loss_kernel's tiling and its two forms with a store in
//                       place of the sums -- prediction read once, gradient written once, gout * sum_k coef_k * term_k in fp32.
//                       The maps form needs no table and no workspace; on sncal_line_target's output it writes the rebuild form's bits.
//   sncal_line_acc_counts   one workgroup; a thread walks (frame, channel) pairs with integer counters, then a fixed-order fold
// exp in the GMSE term is expf (1 ulp), as in loss.hip.  The wing arithmetic is awing.hpp's and the lane / wave helpers are tile.hpp's, both shared with
// loss.hip.
// Nothing here asserts a speed: profiles/validate_line.md holds what was measured against the composed path (sncal_line_target +
// torch ops) at the same commit, and says so where nothing was.
#include "common.hpp"
#include "awing.hpp"
#include "tile.hpp"
#include "../../include/sncal.h"

namespace {

using sncal::Vec;
using sncal::lane_of;
using sncal::wave_sum;

constexpr int LL_MAXC = 64, LS_R = 4, LS_WAVES = 4, LS_ROWS = LS_R * LS_WAVES, LT_ROWS = 32, ACC_MAXT = 8;

// one normalised factor of one point along one axis of n cells; v = the point's coordinate in image pixels
__device__ __forceinline__ float line_gauss1(int i, float v, float flag, float stride, int n, double two_s2) {
    if (flag != 1.0f) return 0.f;
    const float mu = fminf((float)(n - 1), rintf(v / stride));
    const double d = (double)i - (double)mu, m = mu < 0.f ? (double)mu : 0.0;
    return (float)exp(-(d * d - m * m) / two_s2);
}

// keypoint_map += gauss, first point first (0 + a is a)
__device__ __forceinline__ float line_target_value(float gx0, float gy0, float gx1, float gy1) {
    float t = gx0 * gy0;
    t = t + gx1 * gy1;
    return t;
}

__global__ __launch_bounds__(256) void line_target_kernel(const float* __restrict__ kp, float sigma, float stride, int h, int w,
                                                          float* __restrict__ out) {
    __shared__ float s_gy[2][LT_ROWS];
    const int t = threadIdx.x, bc = blockIdx.z, y0 = blockIdx.y * LT_ROWS, x = blockIdx.x * 256 + t;
    const float* const k = kp + (size_t)bc * 6;
    const double two_s2 = 2.0 * (double)sigma * (double)sigma;
    if (t < 2 * LT_ROWS) {
        const int p = t / LT_ROWS, r = t - p * LT_ROWS;
        s_gy[p][r] = y0 + r < h ? line_gauss1(y0 + r, k[p * 3 + 1], k[p * 3 + 2], stride, h, two_s2) : 0.f;
    }
    __syncthreads();
    if (x >= w) return;
    const float gx0 = line_gauss1(x, k[0], k[2], stride, w, two_s2), gx1 = line_gauss1(x, k[3], k[5], stride, w, two_s2);
    const int rows = min(LT_ROWS, h - y0);
    float* const o = out + (size_t)bc * h * w + (size_t)y0 * w + x;
    for (int r = 0; r < rows; ++r) o[(size_t)r * w] = line_target_value(gx0, s_gy[0][r], gx1, s_gy[1][r]);
}

struct Layout { size_t gx, gy, part, total; int bx, by; };

inline Layout layout(int B, int C, int h, int w, int V) {
    Layout L;
    L.bx = (w + 64 * V - 1) / (64 * V);
    L.by = (h + LS_ROWS - 1) / LS_ROWS;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.gx = 0;
    L.gy = up((size_t)B * C * 2 * w * sizeof(float));
    L.part = L.gy + up((size_t)B * C * 2 * h * sizeof(float));
    L.total = L.part + up((size_t)B * L.bx * L.by * 2 * sizeof(double));
    return L;
}

// one workgroup per (frame, channel): gx (B*C, 2, w) and gy (B*C, 2, h)
__global__ __launch_bounds__(256) void line_tables_kernel(const float* __restrict__ kp, float sigma, float stride, int h, int w,
                                                          float* __restrict__ gx, float* __restrict__ gy) {
    const int bc = blockIdx.x;
    const float* const k = kp + (size_t)bc * 6;
    const double two_s2 = 2.0 * (double)sigma * (double)sigma;
    for (int i = threadIdx.x; i < 2 * (w + h); i += 256) {
        const int p = i >= w + h, j = i - p * (w + h);
        if (j < w) gx[((size_t)bc * 2 + p) * w + j] = line_gauss1(j, k[p * 3 + 0], k[p * 3 + 2], stride, w, two_s2);
        else gy[((size_t)bc * 2 + p) * h + (j - w)] = line_gauss1(j - w, k[p * 3 + 1], k[p * 3 + 2], stride, h, two_s2);
    }
}

template <bool REBUILD, int V, bool GMSE, bool AW>
__global__ __launch_bounds__(256) void line_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const float* __restrict__ gxt, const float* __restrict__ gyt, int C, int h, int w,
                                                        float two_gs2, double* __restrict__ part) {
    using VT = typename Vec<V>::type;
    __shared__ float s_gy[REBUILD ? LL_MAXC : 1][2][LS_ROWS];
    __shared__ double s_red[LS_WAVES][2];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.z;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    if (REBUILD) {
        for (int i = t; i < C * 2 * LS_ROWS; i += 256) {
            const int cp = i / LS_ROWS, r = i - cp * LS_ROWS;   // cp = c * 2 + p
            s_gy[cp >> 1][cp & 1][r] = y0 + r < h ? gyt[((size_t)b * C * 2 + cp) * h + y0 + r] : 0.f;
        }
        __syncthreads();
    }
    const int yw = y0 + wv * LS_R;                              // first row of this wave
    const int rows = min(LS_R, h - yw);                         // <= 0: the wave has no row (it still joins the reduction below)
    const bool live = x0 < w && rows > 0;                       // w % V == 0, so a live lane owns V whole columns
    double acc[2] = {0.0, 0.0};
    if (live) {
        const size_t plane = (size_t)h * w, off = (size_t)b * C * plane + (size_t)yw * w + x0;
#pragma unroll 2
        for (int c = 0; c < C; ++c) {
            VT pv[LS_R], tv[LS_R], cx0, cx1;
            if (REBUILD) {
                cx0 = *reinterpret_cast<const VT*>(gxt + ((size_t)b * C + c) * 2 * w + x0);
                cx1 = *reinterpret_cast<const VT*>(gxt + (((size_t)b * C + c) * 2 + 1) * w + x0);
            }
#pragma unroll
            for (int r = 0; r < LS_R; ++r)
                if (r < rows) {
                    pv[r] = *reinterpret_cast<const VT*>(pred + off + (size_t)c * plane + (size_t)r * w);
                    if (!REBUILD) tv[r] = *reinterpret_cast<const VT*>(target + off + (size_t)c * plane + (size_t)r * w);
                }
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < LS_R; ++r) {
                if (r < rows) {
                    float cy0 = 0.f, cy1 = 0.f;
                    if (REBUILD) { cy0 = s_gy[c][0][wv * LS_R + r]; cy1 = s_gy[c][1][wv * LS_R + r]; }
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        const float p = lane_of(pv[r], j);
                        const float tt = REBUILD ? line_target_value(lane_of(cx0, j), cy0, lane_of(cx1, j), cy1) : lane_of(tv[r], j);
                        if (GMSE) {
                            const float d = p - tt, sq = d * d;  // (pred - target) ** 2, times exp(-that / (2 sigma^2))
                            s0 += sq * expf(-sq / two_gs2);
                        }
                        if (AW) s1 += sncal::adaptive_wing(p, tt);
                    }
                }
            }
            acc[0] += (double)s0; acc[1] += (double)s1;
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) s_red[wv][k] = v;
    }
    __syncthreads();
    if (t < 2) {
        double v = 0.0;
        for (int i = 0; i < LS_WAVES; ++i) v += s_red[i][t];
        part[(((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 2 + t] = v;
    }
}

// one thread per (frame, term): the partials of the frame in index order
__global__ void line_fold_kernel(const double* __restrict__ part, int B, int per_frame, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 2) return;
    const int b = i >> 1, k = i & 1;
    double v = 0.0;
    for (int j = 0; j < per_frame; ++j) v += part[((size_t)b * per_frame + j) * 2 + k];
    out[i] = v;
}

template <bool REBUILD, int V>
void launch(int terms, dim3 grid, hipStream_t st, const float* pred, const float* target, const float* gx, const float* gy, int C, int h,
            int w, float two_gs2, double* part) {
#define LL_CASE(T, G, A) case T: hipLaunchKernelGGL((line_loss_kernel<REBUILD, V, G, A>), grid, dim3(256), 0, st, pred, target, gx, gy, C, h, w, two_gs2, part); break;
    switch (terms) { LL_CASE(1, true, false) LL_CASE(2, false, true) LL_CASE(3, true, true) }
#undef LL_CASE
}

struct Coef2 { float c[2]; };

// The tiling, the two forms and the target arithmetic of line_loss_kernel; each element's gradient with respect to the prediction
// is stored where the prediction was read (no sums: no reduction, no partials)
//   d^2 exp(-d^2 / 2s^2), d = p - t   ->  2 d exp(-u) (1 - u),  u = d^2 / 2s^2
//   adaptive_wing(p, t)               ->  w'(|t - p|) sign(p - t)
template <bool REBUILD, int V, bool GMSE, bool AW>
__global__ __launch_bounds__(256) void line_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const float* __restrict__ gxt, const float* __restrict__ gyt, int C, int h, int w,
                                                        float two_gs2, Coef2 cf, const float* __restrict__ gout, float* __restrict__ grad) {
    using VT = typename Vec<V>::type;
    __shared__ float s_gy[REBUILD ? LL_MAXC : 1][2][LS_ROWS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.z;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    if (REBUILD) {
        for (int i = t; i < C * 2 * LS_ROWS; i += 256) {
            const int cp = i / LS_ROWS, r = i - cp * LS_ROWS;   // cp = c * 2 + p
            s_gy[cp >> 1][cp & 1][r] = y0 + r < h ? gyt[((size_t)b * C * 2 + cp) * h + y0 + r] : 0.f;
        }
        __syncthreads();
    }
    const int yw = y0 + wv * LS_R;
    const int rows = min(LS_R, h - yw);
    if (x0 >= w || rows <= 0) return;                           // w % V == 0, so a live lane owns V whole columns
    const float go = gout ? *gout : 1.0f;
    const size_t plane = (size_t)h * w, off = (size_t)b * C * plane + (size_t)yw * w + x0;
#pragma unroll 2
    for (int c = 0; c < C; ++c) {
        VT pv[LS_R], tv[LS_R], cx0, cx1;
        if (REBUILD) {
            cx0 = *reinterpret_cast<const VT*>(gxt + ((size_t)b * C + c) * 2 * w + x0);
            cx1 = *reinterpret_cast<const VT*>(gxt + (((size_t)b * C + c) * 2 + 1) * w + x0);
        }
#pragma unroll
        for (int r = 0; r < LS_R; ++r)
            if (r < rows) {
                pv[r] = *reinterpret_cast<const VT*>(pred + off + (size_t)c * plane + (size_t)r * w);
                if (!REBUILD) tv[r] = *reinterpret_cast<const VT*>(target + off + (size_t)c * plane + (size_t)r * w);
            }
#pragma unroll
        for (int r = 0; r < LS_R; ++r) {
            if (r < rows) {
                float cy0 = 0.f, cy1 = 0.f;
                if (REBUILD) { cy0 = s_gy[c][0][wv * LS_R + r]; cy1 = s_gy[c][1][wv * LS_R + r]; }
                float gv[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float p = lane_of(pv[r], j);
                    const float tt = REBUILD ? line_target_value(lane_of(cx0, j), cy0, lane_of(cx1, j), cy1) : lane_of(tv[r], j);
                    float g = 0.f;
                    if (GMSE) {
                        const float d = p - tt, u = d * d / two_gs2;
                        g += cf.c[0] * (2.0f * d * expf(-u) * (1.0f - u));
                    }
                    if (AW) g += cf.c[1] * sncal::adaptive_wing_grad(p, tt);
                    gv[j] = go * g;
                }
                float* const o = grad + off + (size_t)c * plane + (size_t)r * w;
                if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                else *o = gv[0];
            }
        }
    }
}

template <bool REBUILD, int V>
void launch_grad(int terms, dim3 grid, hipStream_t st, const float* pred, const float* target, const float* gx, const float* gy, int C, int h,
                 int w, float two_gs2, Coef2 cf, const float* gout, float* grad) {
#define LL_CASE(T, G, A) case T: hipLaunchKernelGGL((line_grad_kernel<REBUILD, V, G, A>), grid, dim3(256), 0, st, pred, target, gx, gy, C, h, w, two_gs2, cf, gout, grad); break;
    switch (terms) { LL_CASE(1, true, false) LL_CASE(2, false, true) LL_CASE(3, true, true) }
#undef LL_CASE
}

struct AccTs { float t[ACC_MAXT]; };

// metrics.py:70-98 per (frame, channel); the pairing is by slot index i, the nearest prediction is taken over both slots
__global__ __launch_bounds__(256) void line_acc_kernel(const float* __restrict__ gt, const float* __restrict__ pred, long long items,
                                                       float p_threshold, AccTs ts, int n_t, long long* __restrict__ out) {
    __shared__ long long s_red[LS_WAVES][ACC_MAXT * 3];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    long long cnt[ACC_MAXT][3];
#pragma unroll
    for (int k = 0; k < ACC_MAXT; ++k) cnt[k][0] = cnt[k][1] = cnt[k][2] = 0;
    for (long long it = t; it < items; it += 256) {
        const float* const g = gt + it * 6;
        const float* const p = pred + it * 6;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ge = g[i * 3 + 2] == 1.0f, pe = p[i * 3 + 2] >= p_threshold;
            const float ax = g[i * 3] - p[0], ay = g[i * 3 + 1] - p[1], bx = g[i * 3] - p[3], by = g[i * 3 + 1] - p[4];
            const float d0 = sqrtf(ax * ax + ay * ay), d1 = sqrtf(bx * bx + by * by);
            const float dmin = (d0 != d0 || d1 != d1) ? NAN : fminf(d0, d1);      // torch.min hands a NaN on; NaN <= t is false
#pragma unroll
            for (int k = 0; k < ACC_MAXT; ++k) {
                if (k < n_t) {
                    const bool within = dmin <= ts.t[k];
                    cnt[k][0] += ge && pe && within;
                    cnt[k][1] += (pe && !ge) + (ge && pe && !within);
                    cnt[k][2] += ge && !pe;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < ACC_MAXT; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            long long v = cnt[k][j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if (lane == 0) s_red[wv][k * 3 + j] = v;
        }
    __syncthreads();
    if (t < n_t * 3) {
        long long v = 0;
        for (int i = 0; i < LS_WAVES; ++i) v += s_red[i][t];
        out[t] = v;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sncal_line_target(const float* d_kpts, int B, int C, float sigma, float stride, int h, int w, float* d_out, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && h > 0 && w > 0, "sncal_line_target: B=%d C=%d h=%d w=%d", B, C, h, w);
    SNCAL_CHECK_ARG(sigma > 0.f, "sncal_line_target: sigma %g", (double)sigma);
    SNCAL_CHECK_ARG(stride > 0.f, "sncal_line_target: stride %g", (double)stride);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_kpts && d_out, "sncal_line_target: null pointer");
    SNCAL_CHECK_ARG((long long)B * C <= 65535 && (h + LT_ROWS - 1) / LT_ROWS <= 65535, "sncal_line_target: grid too large");
    hipLaunchKernelGGL(line_target_kernel, dim3((w + 255) / 256, (h + LT_ROWS - 1) / LT_ROWS, B * C), dim3(256), 0, sncal::as_stream(stream),
                       d_kpts, sigma, stride, h, w, d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_line_loss_workspace(int B, int C, int h, int w, size_t* bytes) {
    SNCAL_CHECK_ARG(bytes, "sncal_line_loss_workspace: null pointer");
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && C <= LL_MAXC && h > 0 && w > 0, "sncal_line_loss_workspace: B=%d C=%d h=%d w=%d (C <= %d)", B, C, h, w,
                    LL_MAXC);
    *bytes = layout(B, C, h, w, 1).total;                       // V = 1 has the most partials: enough for either width
    return SNCAL_OK;
}

extern "C" int sncal_line_loss(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w,
                               float target_sigma, float stride, float gmse_sigma, int terms, double* d_out, void* d_ws, size_t ws_bytes,
                               void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && C <= LL_MAXC && h > 0 && w > 0, "sncal_line_loss: B=%d C=%d h=%d w=%d (C <= %d)", B, C, h, w, LL_MAXC);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 3, "sncal_line_loss: terms %d (bit0 gmse, bit1 awing)", terms);
    SNCAL_CHECK_ARG(!(terms & 1) || gmse_sigma > 0.f, "sncal_line_loss: gmse_sigma %g", (double)gmse_sigma);
    if (B == 0) return SNCAL_OK;                                // before the pointers: an empty tensor's is NULL
    SNCAL_CHECK_ARG((d_target != nullptr) != (d_kpts != nullptr), "sncal_line_loss: exactly one of d_target and d_kpts must be given");
    if (d_kpts) {
        SNCAL_CHECK_ARG(target_sigma > 0.f, "sncal_line_loss: target_sigma %g", (double)target_sigma);
        SNCAL_CHECK_ARG(stride > 0.f, "sncal_line_loss: stride %g", (double)stride);
    }
    SNCAL_CHECK_ARG(d_pred && d_out, "sncal_line_loss: null pointer");
    hipStream_t st = sncal::as_stream(stream);
    if (terms == 0) {
        SNCAL_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)B * 2 * sizeof(double), st));
        return SNCAL_OK;
    }
    const int V = (w % 4 == 0 && aligned16(d_pred) && (!d_target || aligned16(d_target))) ? 4 : 1;
    const Layout L = layout(B, C, h, w, V);
    SNCAL_CHECK_ARG(B <= 65535 && L.by <= 65535 && (size_t)B * C <= 0x7fffffffu, "sncal_line_loss: grid too large");
    SNCAL_CHECK_ARG(d_ws && aligned16(d_ws), "sncal_line_loss: workspace pointer null or not 16-byte aligned");
    if (ws_bytes < L.total) {
        sncal::set_error("sncal_line_loss: workspace %zu bytes, need %zu (sncal_line_loss_workspace)", ws_bytes, L.total);
        return SNCAL_ERR_WORKSPACE;
    }
    float* const gx = reinterpret_cast<float*>((char*)d_ws + L.gx);
    float* const gy = reinterpret_cast<float*>((char*)d_ws + L.gy);
    double* const part = reinterpret_cast<double*>((char*)d_ws + L.part);
    const float two_gs2 = 2.0f * gmse_sigma * gmse_sigma;
    const dim3 grid(L.bx, L.by, B);
    if (d_kpts) {
        hipLaunchKernelGGL(line_tables_kernel, dim3(B * C), dim3(256), 0, st, d_kpts, target_sigma, stride, h, w, gx, gy);
        SNCAL_CHECK_LAUNCH();
        if (V == 4) launch<true, 4>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, part);
        else launch<true, 1>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, part);
    } else {
        if (V == 4) launch<false, 4>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, part);
        else launch<false, 1>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, part);
    }
    SNCAL_CHECK_LAUNCH();
    hipLaunchKernelGGL(line_fold_kernel, dim3((B * 2 + 63) / 64), dim3(64), 0, st, part, B, L.bx * L.by, d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_ehm_loss_grad(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w,
                                    float target_sigma, float stride, float gmse_sigma, int terms, const double coef[2],
                                    const float* d_gout, float* d_grad, void* d_ws, size_t ws_bytes, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && C <= LL_MAXC && h > 0 && w > 0, "sncal_ehm_loss_grad: B=%d C=%d h=%d w=%d (C <= %d)", B, C, h, w,
                    LL_MAXC);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 3, "sncal_ehm_loss_grad: terms %d (bit0 gmse, bit1 awing)", terms);
    SNCAL_CHECK_ARG(!(terms & 1) || gmse_sigma > 0.f, "sncal_ehm_loss_grad: gmse_sigma %g", (double)gmse_sigma);
    SNCAL_CHECK_ARG(coef, "sncal_ehm_loss_grad: null coef");
    if (B == 0) return SNCAL_OK;                                // before the pointers: an empty tensor's is NULL
    SNCAL_CHECK_ARG((d_target != nullptr) != (d_kpts != nullptr), "sncal_ehm_loss_grad: exactly one of d_target and d_kpts must be given");
    if (d_kpts) {
        SNCAL_CHECK_ARG(target_sigma > 0.f, "sncal_ehm_loss_grad: target_sigma %g", (double)target_sigma);
        SNCAL_CHECK_ARG(stride > 0.f, "sncal_ehm_loss_grad: stride %g", (double)stride);
    }
    SNCAL_CHECK_ARG(d_pred && d_grad, "sncal_ehm_loss_grad: null pointer");
    hipStream_t st = sncal::as_stream(stream);
    if (terms == 0) {
        SNCAL_CHECK_HIP(hipMemsetAsync(d_grad, 0, (size_t)B * C * h * w * sizeof(float), st));
        return SNCAL_OK;
    }
    const int V = (w % 4 == 0 && aligned16(d_pred) && aligned16(d_grad) && (!d_target || aligned16(d_target))) ? 4 : 1;
    const Layout L = layout(B, C, h, w, V);
    SNCAL_CHECK_ARG(B <= 65535 && L.by <= 65535 && (size_t)B * C <= 0x7fffffffu, "sncal_ehm_loss_grad: grid too large");
    const float two_gs2 = 2.0f * gmse_sigma * gmse_sigma;
    const Coef2 cf = {{(float)coef[0], (float)coef[1]}};
    const dim3 grid(L.bx, L.by, B);
    if (d_kpts) {
        SNCAL_CHECK_ARG(d_ws && aligned16(d_ws), "sncal_ehm_loss_grad: workspace pointer null or not 16-byte aligned");
        if (ws_bytes < L.part) {                                // the tables only: no partial sums here
            sncal::set_error("sncal_ehm_loss_grad: workspace %zu bytes, need %zu (sncal_line_loss_workspace covers it)", ws_bytes, L.part);
            return SNCAL_ERR_WORKSPACE;
        }
        float* const gx = reinterpret_cast<float*>((char*)d_ws + L.gx);
        float* const gy = reinterpret_cast<float*>((char*)d_ws + L.gy);
        hipLaunchKernelGGL(line_tables_kernel, dim3(B * C), dim3(256), 0, st, d_kpts, target_sigma, stride, h, w, gx, gy);
        SNCAL_CHECK_LAUNCH();
        if (V == 4) launch_grad<true, 4>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, cf, d_gout, d_grad);
        else launch_grad<true, 1>(terms, grid, st, d_pred, d_target, gx, gy, C, h, w, two_gs2, cf, d_gout, d_grad);
    } else {                                                    // the maps form needs no table, hence no workspace
        if (V == 4) launch_grad<false, 4>(terms, grid, st, d_pred, d_target, nullptr, nullptr, C, h, w, two_gs2, cf, d_gout, d_grad);
        else launch_grad<false, 1>(terms, grid, st, d_pred, d_target, nullptr, nullptr, C, h, w, two_gs2, cf, d_gout, d_grad);
    }
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_line_acc_counts(const float* d_gt, const float* d_pred, int B, int C, float p_threshold, const float* ts, int n_t,
                                     long long* d_out, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && C > 0, "sncal_line_acc_counts: B=%d C=%d", B, C);
    SNCAL_CHECK_ARG(n_t > 0 && n_t <= ACC_MAXT, "sncal_line_acc_counts: n_t %d (1..%d thresholds)", n_t, ACC_MAXT);
    SNCAL_CHECK_ARG(ts && d_out, "sncal_line_acc_counts: null pointer");
    SNCAL_CHECK_ARG(B == 0 || (d_gt && d_pred), "sncal_line_acc_counts: null pointer");
    AccTs a;
    for (int k = 0; k < ACC_MAXT; ++k) a.t[k] = k < n_t ? ts[k] : 0.f;
    hipLaunchKernelGGL(line_acc_kernel, dim3(1), dim3(256), 0, sncal::as_stream(stream), d_gt, d_pred, (long long)B * C, p_threshold, a, n_t,
                       d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
