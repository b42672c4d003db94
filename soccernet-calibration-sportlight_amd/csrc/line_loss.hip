// The loss and validation tail of the line model: the two-peak target maps, EHMLoss.forward for num_refinement_stages = 0 in ONE
// read of the softmax heatmap, its gradient in one more read and one write, and the tp / fp / fn counts of AccMetric
//   /root/reference/src/models/line/dataset.py:107-178 (_generate_keypoint_maps, _add_gaussian)
//   /root/reference/src/models/line/loss.py:34-108     (forward, gmse_loss, adaptive_wing)
//   /root/reference/src/models/line/metrics.py:53-103  (a_t_score)
// Target: a channel holds up to two Gaussians, centred on mu = (min(w-1, rint(x/stride)), min(h-1, rint(y/stride))) (fp32
// division, ties to even, no lower clamp) and divided by their maximum over the grid.  Both are separable, and so is the maximum
// (1 unless mu < 0, then the value at index 0), so one factor is
//     g[i] = exp(-((i - mu)^2 - min(mu, 0)^2) / (2 sigma^2)),     evaluated in fp64 and rounded once (line_gauss1)
// and an element is gx0[x]*gy0[y] + gx1[x]*gy1[y] in fp32, first point first (loss_frame.hpp: line_target_value).  A point whose
// flag is not 1 has all-zero factors.
//   sncal_line_target   a thread owns one column of a 32-row strip of one channel: its two column factors in registers, the
//                       strip's row factors in LDS; 2*(w + 32) exps per 32*w stores
//   sncal_line_loss     line_tables_kernel writes the factors of every (frame, channel) to the workspace once; line_loss_kernel is
//                       loss_frame.hpp's walk with its sum sink and the two terms of LineSums below, on the rebuild model
//                       (REBUILD = true) or the maps model (false: the target read from memory, as a loader delivers it; fed with
//                       sncal_line_target's output it sees the very values the rebuild model forms, in the same order); the
//                       frame's fold kernel adds the partials of a frame in index order.
//   sncal_ehm_loss_grad    the gradient of that loss with respect to the prediction (torch autograd through line/loss.py:61-108,
//                       the target held fixed): line_grad_kernel is the same walk and models with the frame's store sink and
//                       LineGrad below -- prediction read once, gradient written once, gout * sum_k coef_k * term_k in fp32.
//                       The maps form needs no table and no workspace; on sncal_line_target's output it writes the rebuild form's bits.
//   sncal_line_acc_counts   one workgroup; a thread walks (frame, channel) pairs with integer counters, then a fixed-order fold
// exp in the GMSE term is expf (1 ulp), as in loss.hip.  The wing arithmetic is awing.hpp's, shared with loss.hip.
// Nothing here asserts a speed: profiles/validate_line.md holds what was measured against the composed path (sncal_line_target +
// torch ops) at the same commit, and says so where nothing was.
#include "common.hpp"
#include "awing.hpp"
#include "loss_frame.hpp"
#include "../../include/sncal.h"

using namespace sncal;                                          // loss_frame.hpp: tiling, walk, models, sinks, host prologue

namespace {

constexpr int LT_ROWS = 32, ACC_MAXT = 8;

// one normalised factor of one point along one axis of n cells; v = the point's coordinate in image pixels
__device__ __forceinline__ float line_gauss1(int i, float v, float flag, float stride, int n, double two_s2) {
    if (flag != 1.0f) return 0.f;
    const float mu = fminf((float)(n - 1), rintf(v / stride));
    const double d = (double)i - (double)mu, m = mu < 0.f ? (double)mu : 0.0;
    return (float)exp(-(d * d - m * m) / two_s2);
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

// the two terms of one element, p the prediction, t the target
template <bool GMSE, bool AW>
struct LineSums {
    static constexpr int K = 2;
    float two_gs2;
    __device__ __forceinline__ void sum(float p, float t, float, float (&s)[2]) const {
        if (GMSE) {
            const float d = p - t, sq = d * d;                  // (pred - target) ** 2, times exp(-that / (2 sigma^2))
            s[0] += sq * expf(-sq / two_gs2);
        }
        if (AW) s[1] += adaptive_wing(p, t);
    }
};

// their derivatives with respect to the prediction
//   d^2 exp(-d^2 / 2s^2), d = p - t   ->  2 d exp(-u) (1 - u),  u = d^2 / 2s^2
//   adaptive_wing(p, t)               ->  w'(|t - p|) sign(p - t)
template <bool GMSE, bool AW>
struct LineGrad {
    float two_gs2, c[2];
    __device__ __forceinline__ float grad(float p, float t) const {
        float g = 0.f;
        if (GMSE) {
            const float d = p - t, u = d * d / two_gs2;
            g += c[0] * (2.0f * d * expf(-u) * (1.0f - u));
        }
        if (AW) g += c[1] * adaptive_wing_grad(p, t);
        return g;
    }
};

// the frame's walk on the rebuild model (tables in the workspace) or on the maps model (the target in memory)
template <bool REBUILD, int V, class Sink>
__device__ __forceinline__ void line_walk(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ gxt,
                                          const float* __restrict__ gyt, int C, int h, int w, Sink& sink) {
    if constexpr (REBUILD) {
        LineRebuildModel<V> model{gxt, gyt, C};
        loss_walk<V>(pred, C, h, w, model, sink);
    } else {
        LineMapsModel<V> model{target};
        loss_walk<V>(pred, C, h, w, model, sink);
    }
}

template <bool REBUILD, int V, bool GMSE, bool AW>
__global__ __launch_bounds__(256) void line_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const float* __restrict__ gxt, const float* __restrict__ gyt, int C, int h, int w,
                                                        LineSums<GMSE, AW> terms, double* __restrict__ part) {
    SumSink<LineSums<GMSE, AW>> sink{terms, part};
    line_walk<REBUILD, V>(pred, target, gxt, gyt, C, h, w, sink);
}

template <bool REBUILD, int V, bool GMSE, bool AW>
__global__ __launch_bounds__(256) void line_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const float* __restrict__ gxt, const float* __restrict__ gyt, int C, int h, int w,
                                                        LineGrad<GMSE, AW> terms, const float* __restrict__ gout, float* __restrict__ grad) {
    StoreSink<V, LineGrad<GMSE, AW>> sink{terms, gout, grad};
    line_walk<REBUILD, V>(pred, target, gxt, gyt, C, h, w, sink);
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

constexpr LossShape shape(int B, int C, int h, int w) { return {B, C, h, w, 2 * sizeof(float), 2}; }

// the checks of both entry points up to the pointers, in the order the header documents; B == 0 ends them before any pointer is
// looked at (an empty tensor's is NULL), and the caller returns
int check(const char* fn, int B, int C, int h, int w, int terms, float gmse_sigma, bool coef_ok, const float* d_target, const float* d_kpts,
          float target_sigma, float stride) {
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && C <= LS_MAXC && h > 0 && w > 0, "%s: B=%d C=%d h=%d w=%d (C <= %d)", fn, B, C, h, w, LS_MAXC);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 3, "%s: terms %d (bit0 gmse, bit1 awing)", fn, terms);
    SNCAL_CHECK_ARG(!(terms & 1) || gmse_sigma > 0.f, "%s: gmse_sigma %g", fn, (double)gmse_sigma);
    SNCAL_CHECK_ARG(coef_ok, "%s: null coef", fn);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG((d_target != nullptr) != (d_kpts != nullptr), "%s: exactly one of d_target and d_kpts must be given", fn);
    if (d_kpts) {
        SNCAL_CHECK_ARG(target_sigma > 0.f, "%s: target_sigma %g", fn, (double)target_sigma);
        SNCAL_CHECK_ARG(stride > 0.f, "%s: stride %g", fn, (double)stride);
    }
    return SNCAL_OK;
}

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
    SNCAL_CHECK_ARG(B >= 0 && C > 0 && C <= LS_MAXC && h > 0 && w > 0, "sncal_line_loss_workspace: B=%d C=%d h=%d w=%d (C <= %d)", B, C, h, w,
                    LS_MAXC);
    *bytes = loss_workspace_bytes(shape(B, C, h, w));
    return SNCAL_OK;
}

extern "C" int sncal_line_loss(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w,
                               float target_sigma, float stride, float gmse_sigma, int terms, double* d_out, void* d_ws, size_t ws_bytes,
                               void* stream) {
    static const char fn[] = "sncal_line_loss";
    int rc = check(fn, B, C, h, w, terms, gmse_sigma, true, d_target, d_kpts, target_sigma, stride);
    if (rc != SNCAL_OK || B == 0) return rc;
    SNCAL_CHECK_ARG(d_pred && d_out, "%s: null pointer", fn);
    LossLaunch L;
    rc = loss_prologue(L, fn, "sncal_line_loss_workspace", shape(B, C, h, w), terms, d_out, (size_t)B * 2 * sizeof(double),
                       aligned16({d_pred, d_target}), LOSS_WS_ALL, d_ws, ws_bytes, stream);
    if (rc != SNCAL_OK || L.done) return rc;
    float* const gx = static_cast<float*>(L.gx);
    float* const gy = static_cast<float*>(L.gy);
    if (d_kpts) {
        hipLaunchKernelGGL(line_tables_kernel, dim3(B * C), dim3(256), 0, L.st, d_kpts, target_sigma, stride, h, w, gx, gy);
        SNCAL_CHECK_LAUNCH();
    }
    loss_dispatch<3>(terms, L.V, [&](auto T, auto V) {
        constexpr int t = decltype(T)::value, v = decltype(V)::value;
        const LineSums<(t & 1) != 0, (t & 2) != 0> ts = {2.0f * gmse_sigma * gmse_sigma};
        if (d_kpts) hipLaunchKernelGGL((line_loss_kernel<true, v, (t & 1) != 0, (t & 2) != 0>), L.grid, dim3(256), 0, L.st, d_pred, d_target, gx, gy, C, h, w, ts, L.part);
        else hipLaunchKernelGGL((line_loss_kernel<false, v, (t & 1) != 0, (t & 2) != 0>), L.grid, dim3(256), 0, L.st, d_pred, d_target, gx, gy, C, h, w, ts, L.part);
    });
    SNCAL_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_fold_kernel<2>, dim3((B * 2 + 63) / 64), dim3(64), 0, L.st, L.part, B, L.per_frame, d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_ehm_loss_grad(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w,
                                    float target_sigma, float stride, float gmse_sigma, int terms, const double coef[2],
                                    const float* d_gout, float* d_grad, void* d_ws, size_t ws_bytes, void* stream) {
    static const char fn[] = "sncal_ehm_loss_grad";
    int rc = check(fn, B, C, h, w, terms, gmse_sigma, coef != nullptr, d_target, d_kpts, target_sigma, stride);
    if (rc != SNCAL_OK || B == 0) return rc;
    SNCAL_CHECK_ARG(d_pred && d_grad, "%s: null pointer", fn);
    LossLaunch L;                                               // the maps form needs no table, hence no workspace
    rc = loss_prologue(L, fn, "sncal_line_loss_workspace", shape(B, C, h, w), terms, d_grad, (size_t)B * C * h * w * sizeof(float),
                       aligned16({d_pred, d_target, d_grad}), d_kpts ? LOSS_WS_TABLES : LOSS_WS_NONE, d_ws, ws_bytes, stream);
    if (rc != SNCAL_OK || L.done) return rc;
    float* const gx = static_cast<float*>(L.gx);
    float* const gy = static_cast<float*>(L.gy);
    if (d_kpts) {
        hipLaunchKernelGGL(line_tables_kernel, dim3(B * C), dim3(256), 0, L.st, d_kpts, target_sigma, stride, h, w, gx, gy);
        SNCAL_CHECK_LAUNCH();
    }
    loss_dispatch<3>(terms, L.V, [&](auto T, auto V) {
        constexpr int t = decltype(T)::value, v = decltype(V)::value;
        const LineGrad<(t & 1) != 0, (t & 2) != 0> ts = {2.0f * gmse_sigma * gmse_sigma, {(float)coef[0], (float)coef[1]}};
        if (d_kpts) hipLaunchKernelGGL((line_grad_kernel<true, v, (t & 1) != 0, (t & 2) != 0>), L.grid, dim3(256), 0, L.st, d_pred, d_target, gx, gy, C, h, w, ts, d_gout, d_grad);
        else hipLaunchKernelGGL((line_grad_kernel<false, v, (t & 1) != 0, (t & 2) != 0>), L.grid, dim3(256), 0, L.st, d_pred, d_target, gx, gy, C, h, w, ts, d_gout, d_grad);
    });
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
