// Fused validation loss: HRNetLoss.forward for num_refinement_stages = 0 in ONE read of the log-probability heatmap
//   /root/reference/src/models/hrnet/loss.py:89-119 (forward), :129-144 (adaptive_wing), :76-79 (its constants)
// d_logp (B,N+1,h,w) fp32 log-probabilities, d_kpts (B,N,3) [x, y, flag] in IMAGE pixels, d_mask (B,N+1) or NULL
//   -> d_out (B,3) fp64: per-frame SUMS over (N+1)*h*w of   (exp(p) - t)^2,   xlogy(t, t) - t*p,   adaptive_wing(exp(p), t)
// where p = logp * mask and t = target * mask (loss.py:94-103).  The host divides (MSELoss mean, KLDiv batchmean, torch.mean).
//
// The target is never written: it is separable, t[n][y][x] = gx[n][x] * gy[n][y], so
//   1. loss_tables_kernel evaluates the N*(w + h) Gaussians of a frame once (gauss.hpp: the arithmetic of target.hip, correctly
//      rounded exp) into the workspace, each with the exp's fp32 argument beside it; keypoints are divided by `stride` in fp32
//      first (loss.py:92) and the visibility test runs on the divided values, as in the reference;
//   2. loss_kernel walks the heatmap once: loss_frame.hpp's tiling and walk, its keypoint model (the N Gaussian channels, then the
//      background channel 1 - running max) and its sum sink with the three terms of HeatSums below;
//   3. the frame's fold kernel adds the partials of a frame in index order.  No atomics anywhere: two runs give the same bits.
// Logarithm of the target (KL term): ANALYTIC on the keypoint channels with mask == 1, log t = ax + ay, the sum of the two exp
// arguments (the reference takes log of the fp32 product gx * gy; the two differ by the roundings of gx, gy and the product, below
// 2e-7 absolute, and where the product underflowed to 0 the term is 0 either way).  The background channel and channels whose mask
// is neither 0 nor 1 take a real logf.  exp of the prediction is expf (1 ulp), not the fast intrinsic: the intrinsic's argument
// scaling is biased by the rounding of log2(e), which does not average out over a sum.
// Gradient (sncal_heatmap_loss_grad, what torch autograd gives through loss.py:89-144 with the target held fixed): the losses are
// elementwise given the tables, so loss_grad_kernel is the same walk and model with the frame's store sink and HeatGrad below --
// the prediction read once, the gradient written once, the background channel's last because its target needs the running max.
// grad = gout * m * sum_k coef_k * term_k in fp32, coef_k = weight / divisor from the host.  What was measured is in
// profiles/loss_grad.md.
// Cost per element with the default terms: one expf + about a dozen fp32 ops and a share of a float2 table load.  Which of HBM
// or VALU issue bounds each variant is a question for measurement, not for this header: profiles/validate_loss.md holds what was
// measured (kernel times from a trace, algorithmic bytes over time against the HBM rate) and says so where nothing was.
#include "common.hpp"
#include "awing.hpp"
#include "loss_frame.hpp"
#include "gauss.hpp"
#include "../../include/sncal.h"

using namespace sncal;                                          // loss_frame.hpp: tiling, walk, models, sinks, host prologue

namespace {

// one workgroup per (frame, keypoint): {Gaussian, its exp argument} for every column and every row; {0, 0} where not visible
__global__ __launch_bounds__(256) void loss_tables_kernel(const float* __restrict__ kp, int N, float sigma, float stride, int h, int w,
                                                          float2* __restrict__ gx, float2* __restrict__ gy) {
    const int bn = blockIdx.x;                                  // b * N + n
    const float x = kp[(size_t)bn * 3 + 0] / stride, y = kp[(size_t)bn * 3 + 1] / stride, f = kp[(size_t)bn * 3 + 2];
    const bool vis = sncal::kp_visible(x, y, f);
    for (int i = threadIdx.x; i < w + h; i += 256) {
        const bool col = i < w;
        const float a = sncal::gauss1_arg((float)(col ? i : i - w), col ? x : y, sigma);
        const float2 v = vis ? make_float2((float)exp((double)a), a) : make_float2(0.f, 0.f);
        if (col) gx[(size_t)bn * w + i] = v; else gy[(size_t)bn * h + (i - w)] = v;
    }
}

// the three terms of one element, p the masked log-probability, t the masked target, logt its logarithm (used by KL alone)
template <bool MSE, bool KL, bool AW>
struct HeatSums {
    static constexpr int K = 3;
    __device__ __forceinline__ void sum(float p, float t, float logt, float (&s)[3]) const {
        const float e = expf(p);                                // pred_01 = torch.exp(pred_masked)
        if (MSE) { const float d = e - t; s[0] = fmaf(d, d, s[0]); }
        if (KL) s[1] += t > 0.f ? t * (logt - p) : 0.f;         // xlogy(t, t) - t * p; target 0 contributes 0 (t is never negative)
        if (AW) s[2] += adaptive_wing(e, t);                    // awing.hpp, shared with line_loss.hip
    }
};

// d/dx of the three terms at one element, x the logit, p = x * m, t = target * m; the common factor m is the model's chain()
//   (exp(p) - t)^2          ->  2 (e - t) e
//   xlogy(t, t) - t p       ->  -t                       (0 where t = 0)
//   adaptive_wing(e, t)     ->  w'(|t - e|) sign(e - t) e
template <bool MSE, bool KL, bool AW>
struct HeatGrad {
    float c[3];
    __device__ __forceinline__ float grad(float p, float t) const {
        const float e = expf(p);
        float g = 0.f;
        if (MSE) g += c[0] * (2.0f * (e - t) * e);
        if (KL) g += c[1] * -t;
        if (AW) g += c[2] * (adaptive_wing_grad(e, t) * e);
        return g;
    }
};

template <int V, bool MSE, bool KL, bool AW>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ logp, const float* __restrict__ mask,
                                                   const float2* __restrict__ gxt, const float2* __restrict__ gyt, int N, int h, int w,
                                                   double* __restrict__ part) {
    KeypointModel<V, KL> model{mask, gxt, gyt, N};
    SumSink<HeatSums<MSE, KL, AW>> sink{{}, part};
    loss_walk<V>(logp, N + 1, h, w, model, sink);
}

// All three terms on the 16-byte path: the one instantiation without a register to spare (124 VGPRs, 4 waves per SIMD).  Through the
// frame it has the same instructions in another order and measured 1 % slower (profiles/loss_frame.md), so it keeps the walk
// written out: the frame's tiling, staging, target and order of sums, statement by statement.
template <>
__global__ __launch_bounds__(256) void loss_kernel<4, true, true, true>(const float* __restrict__ logp, const float* __restrict__ mask,
                                                                       const float2* __restrict__ gxt, const float2* __restrict__ gyt,
                                                                       int N, int h, int w, double* __restrict__ part) {
    constexpr int V = 4;
    __shared__ float2 s_gy[LS_MAXC][LS_ROWS];
    __shared__ float s_m[LS_MAXC + 1];
    __shared__ double s_red[LS_WAVES][3];
    const HeatSums<true, true, true> terms = {};
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.z;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    for (int i = t; i < N * LS_ROWS; i += 256) {
        const int n = i / LS_ROWS, r = i - n * LS_ROWS;
        s_gy[n][r] = y0 + r < h ? gyt[((size_t)b * N + n) * h + y0 + r] : make_float2(0.f, 0.f);
    }
    for (int i = t; i <= N; i += 256) s_m[i] = mask ? mask[(size_t)b * (N + 1) + i] : 1.0f;
    __syncthreads();
    const int yw = y0 + wv * LS_R, rows = min(LS_R, h - yw);
    const bool live = x0 < w && rows > 0;
    double acc[3] = {0.0, 0.0, 0.0};
    if (live) {
        const size_t plane = (size_t)h * w;
        const float* const base = logp + (size_t)b * (N + 1) * plane + (size_t)yw * w + x0;
        float mx[LS_R][V];
#pragma unroll
        for (int r = 0; r < LS_R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) mx[r][j] = 0.f;
#pragma unroll 2
        for (int n = 0; n <= N; ++n) {
            const bool bg = n == N;
            const float m = s_m[n];
            float2 cx[V];
            if (!bg) {
#pragma unroll
                for (int j = 0; j < V; ++j) cx[j] = gxt[((size_t)b * N + n) * w + x0 + j];
            }
            float4 pv[LS_R];
#pragma unroll
            for (int r = 0; r < LS_R; ++r)
                if (r < rows) pv[r] = *reinterpret_cast<const float4*>(base + (size_t)n * plane + (size_t)r * w);
            float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < LS_R; ++r) {
                if (r < rows) {
                    const float2 cy = bg ? make_float2(0.f, 0.f) : s_gy[n][wv * LS_R + r];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float p = lane_of(pv[r], j), tt, lt;
                        if (!bg) {
                            tt = cx[j].x * cy.x;
                            mx[r][j] = fmaxf(mx[r][j], tt);
                            lt = cx[j].y + cy.y;
                        } else {
                            tt = 1.0f - mx[r][j];
                            lt = 0.f;
                        }
                        if (m != 1.0f) { p *= m; tt *= m; }
                        if (bg || m != 1.0f) lt = logf(tt);
                        terms.sum(p, tt, lt, s);
                    }
                }
            }
            acc[0] += (double)s[0]; acc[1] += (double)s[1]; acc[2] += (double)s[2];
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) s_red[wv][k] = v;
    }
    __syncthreads();
    if (t < 3) {
        double v = 0.0;
        for (int i = 0; i < LS_WAVES; ++i) v += s_red[i][t];
        part[(((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3 + t] = v;
    }
}

template <int V, bool MSE, bool KL, bool AW>
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ logp, const float* __restrict__ mask,
                                                        const float2* __restrict__ gxt, const float2* __restrict__ gyt, int N, int h, int w,
                                                        HeatGrad<MSE, KL, AW> terms, const float* __restrict__ gout, float* __restrict__ grad) {
    KeypointModel<V, false> model{mask, gxt, gyt, N};
    StoreSink<V, HeatGrad<MSE, KL, AW>> sink{terms, gout, grad};
    loss_walk<V>(logp, N + 1, h, w, model, sink);
}

constexpr LossShape shape(int B, int N, int h, int w) { return {B, N, h, w, sizeof(float2), 3}; }

// the checks of both entry points up to the pointers, in the order the header documents
int check(const char* fn, int B, int N, int h, int w, float sigma, float stride, int terms, bool coef_ok) {
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= LS_MAXC && h > 0 && w > 0, "%s: B=%d N=%d h=%d w=%d (N <= %d)", fn, B, N, h, w, LS_MAXC);
    SNCAL_CHECK_ARG(sigma > 0.f, "%s: sigma %g", fn, (double)sigma);
    SNCAL_CHECK_ARG(stride > 0.f, "%s: stride %g", fn, (double)stride);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 7, "%s: terms %d (bit0 mse, bit1 kl, bit2 awing)", fn, terms);
    SNCAL_CHECK_ARG(coef_ok, "%s: null coef", fn);
    return SNCAL_OK;
}

}  // namespace

extern "C" int sncal_heatmap_loss_workspace(int B, int N, int h, int w, size_t* bytes) {
    SNCAL_CHECK_ARG(bytes, "sncal_heatmap_loss_workspace: null pointer");
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= LS_MAXC && h > 0 && w > 0, "sncal_heatmap_loss_workspace: B=%d N=%d h=%d w=%d (N <= %d)", B, N, h, w,
                    LS_MAXC);
    *bytes = loss_workspace_bytes(shape(B, N, h, w));
    return SNCAL_OK;
}

extern "C" int sncal_heatmap_loss(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w, float sigma,
                                  float stride, int terms, double* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    static const char fn[] = "sncal_heatmap_loss";
    int rc = check(fn, B, N, h, w, sigma, stride, terms, true);
    if (rc != SNCAL_OK || B == 0) return rc;                    // B == 0 before the pointers: an empty tensor's is NULL
    SNCAL_CHECK_ARG(d_logp && d_kpts && d_out, "%s: null pointer", fn);
    LossLaunch L;
    rc = loss_prologue(L, fn, "sncal_heatmap_loss_workspace", shape(B, N, h, w), terms, d_out, (size_t)B * 3 * sizeof(double),
                       aligned16({d_logp}), LOSS_WS_ALL, d_ws, ws_bytes, stream);
    if (rc != SNCAL_OK || L.done) return rc;
    float2* const gx = static_cast<float2*>(L.gx);
    float2* const gy = static_cast<float2*>(L.gy);
    hipLaunchKernelGGL(loss_tables_kernel, dim3(B * N), dim3(256), 0, L.st, d_kpts, N, sigma, stride, h, w, gx, gy);
    SNCAL_CHECK_LAUNCH();
    loss_dispatch<7>(terms, L.V, [&](auto T, auto V) {
        constexpr int t = decltype(T)::value;
        hipLaunchKernelGGL((loss_kernel<decltype(V)::value, (t & 1) != 0, (t & 2) != 0, (t & 4) != 0>), L.grid, dim3(256), 0, L.st, d_logp, d_mask,
                           gx, gy, N, h, w, L.part);
    });
    SNCAL_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_fold_kernel<3>, dim3((B * 3 + 63) / 64), dim3(64), 0, L.st, L.part, B, L.per_frame, d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_heatmap_loss_grad(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w,
                                       float sigma, float stride, int terms, const double coef[3], const float* d_gout, float* d_grad,
                                       void* d_ws, size_t ws_bytes, void* stream) {
    static const char fn[] = "sncal_heatmap_loss_grad";
    int rc = check(fn, B, N, h, w, sigma, stride, terms, coef != nullptr);
    if (rc != SNCAL_OK || B == 0) return rc;
    SNCAL_CHECK_ARG(d_logp && d_kpts && d_grad, "%s: null pointer", fn);
    LossLaunch L;
    rc = loss_prologue(L, fn, "sncal_heatmap_loss_workspace", shape(B, N, h, w), terms, d_grad, (size_t)B * (N + 1) * h * w * sizeof(float),
                       aligned16({d_logp, d_grad}), LOSS_WS_TABLES, d_ws, ws_bytes, stream);
    if (rc != SNCAL_OK || L.done) return rc;
    float2* const gx = static_cast<float2*>(L.gx);
    float2* const gy = static_cast<float2*>(L.gy);
    hipLaunchKernelGGL(loss_tables_kernel, dim3(B * N), dim3(256), 0, L.st, d_kpts, N, sigma, stride, h, w, gx, gy);
    SNCAL_CHECK_LAUNCH();
    loss_dispatch<7>(terms, L.V, [&](auto T, auto V) {
        constexpr int t = decltype(T)::value;
        const HeatGrad<(t & 1) != 0, (t & 2) != 0, (t & 4) != 0> cf = {{(float)coef[0], (float)coef[1], (float)coef[2]}};
        hipLaunchKernelGGL((loss_grad_kernel<decltype(V)::value, (t & 1) != 0, (t & 2) != 0, (t & 4) != 0>), L.grid, dim3(256), 0, L.st, d_logp,
                           d_mask, gx, gy, N, h, w, cf, d_gout, d_grad);
    });
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
