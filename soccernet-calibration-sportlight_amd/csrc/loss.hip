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
//   2. loss_kernel: a workgroup of 4 waves owns a tile of 4*LS_R rows x 64*V columns of one frame, a lane owns V consecutive
//      columns (V = 4: 16-byte loads, when w % 4 == 0 and the base is 16-byte aligned; V = 1 otherwise) of LS_R rows.  It walks the
//      N keypoint channels (column Gaussians from the table, L2-resident; row Gaussians from LDS), keeps the running max for the
//      background channel 1 - max in registers, sums each channel's LS_R*V elements in fp32 and folds that into three fp64
//      accumulators per lane; wave shuffle -> LDS -> one partial per workgroup in the workspace;
//   3. loss_fold_kernel adds the partials of a frame in index order.  No atomics anywhere: two runs give the same bits.
// Logarithm of the target (KL term): ANALYTIC on the keypoint channels with mask == 1, log t = ax + ay, the sum of the two exp
// arguments (the reference takes log of the fp32 product gx * gy; the two differ by the roundings of gx, gy and the product, below
// 2e-7 absolute, and where the product underflowed to 0 the term is 0 either way).  The background channel and channels whose mask
// is neither 0 nor 1 take a real logf.  exp of the prediction is expf (1 ulp), not the fast intrinsic: the intrinsic's argument
// scaling is biased by the rounding of log2(e), which does not average out over a sum.
// Gradient (sncal_heatmap_loss_grad, what torch autograd gives through loss.py:89-144 with the target held fixed): the losses are
// elementwise given the tables, so loss_grad_kernel is loss_kernel's tiling and channel walk with a store in place of the sums --
// the prediction read once, the gradient written once (16-byte stores when V = 4), the background channel's last because its target
// needs the running max.  grad = gout * m * sum_k coef_k * term_k in fp32, coef_k = weight / divisor from the host, gout a device
// scalar (NULL = 1).  No partials, no fold, no atomics.  What was measured is in profiles/loss_grad.md.
// Cost per element with the default terms: one expf + about a dozen fp32 ops and a share of a float2 table load.  Which of HBM
// or VALU issue bounds each variant is a question for measurement, not for this header: profiles/validate_loss.md holds what was
// measured (kernel times from a trace, algorithmic bytes over time against the HBM rate) and says so where nothing was.
#include "common.hpp"
#include "awing.hpp"
#include "tile.hpp"
#include "gauss.hpp"
#include "../../include/sncal.h"

namespace {

using sncal::Vec;
using sncal::lane_of;
using sncal::wave_sum;

constexpr int LS_MAXN = 64, LS_R = 4, LS_WAVES = 4, LS_ROWS = LS_R * LS_WAVES;

struct Layout { size_t gx, gy, part, total; int bx, by; };

inline Layout layout(int B, int N, int h, int w, int V) {
    Layout L;
    L.bx = (w + 64 * V - 1) / (64 * V);
    L.by = (h + LS_ROWS - 1) / LS_ROWS;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.gx = 0;
    L.gy = up((size_t)B * N * w * sizeof(float2));
    L.part = L.gy + up((size_t)B * N * h * sizeof(float2));
    L.total = L.part + up((size_t)B * L.bx * L.by * 3 * sizeof(double));
    return L;
}

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

template <bool MSE, bool KL, bool AW>
__device__ __forceinline__ void element(float p, float t, float logt, float& s_mse, float& s_kl, float& s_aw) {
    const float e = expf(p);                                    // pred_01 = torch.exp(pred_masked)
    if (MSE) { const float d = e - t; s_mse = fmaf(d, d, s_mse); }
    if (KL) s_kl += t > 0.f ? t * (logt - p) : 0.f;             // xlogy(t, t) - t * p; target 0 contributes 0 (t is never negative)
    if (AW) s_aw += sncal::adaptive_wing(e, t);                 // awing.hpp, shared with line_loss.hip
}

template <int V, bool MSE, bool KL, bool AW>
__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ logp, const float* __restrict__ mask,
                                                   const float2* __restrict__ gxt, const float2* __restrict__ gyt, int N, int h, int w,
                                                   double* __restrict__ part) {
    using VT = typename Vec<V>::type;
    __shared__ float2 s_gy[LS_MAXN][LS_ROWS];
    __shared__ float s_m[LS_MAXN + 1];
    __shared__ double s_red[LS_WAVES][3];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.z;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    for (int i = t; i < N * LS_ROWS; i += 256) {
        const int n = i / LS_ROWS, r = i - n * LS_ROWS;
        s_gy[n][r] = y0 + r < h ? gyt[((size_t)b * N + n) * h + y0 + r] : make_float2(0.f, 0.f);
    }
    for (int i = t; i <= N; i += 256) s_m[i] = mask ? mask[(size_t)b * (N + 1) + i] : 1.0f;
    __syncthreads();
    const int yw = y0 + wv * LS_R;                              // first row of this wave
    const int rows = min(LS_R, h - yw);                         // <= 0: the wave has no row (it still joins the reduction below)
    const bool live = x0 < w && rows > 0;                       // w % V == 0, so a live lane owns V whole columns
    double acc[3] = {0.0, 0.0, 0.0};
    if (live) {
        const size_t plane = (size_t)h * w;
        const float* const base = logp + (size_t)b * (N + 1) * plane + (size_t)yw * w + x0;
        float mx[LS_R][V];
#pragma unroll
        for (int r = 0; r < LS_R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) mx[r][j] = 0.f;         // targets are >= 0 and N >= 1: the same max as torch.max over the channels
#pragma unroll 2
        for (int n = 0; n <= N; ++n) {
            const bool bg = n == N;
            const float m = s_m[n];
            float2 cx[V];
            if (!bg) {
#pragma unroll
                for (int j = 0; j < V; ++j) cx[j] = gxt[((size_t)b * N + n) * w + x0 + j];
            }
            VT pv[LS_R];
#pragma unroll
            for (int r = 0; r < LS_R; ++r)
                if (r < rows) pv[r] = *reinterpret_cast<const VT*>(base + (size_t)n * plane + (size_t)r * w);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int r = 0; r < LS_R; ++r) {
                if (r < rows) {
                    const float2 cy = bg ? make_float2(0.f, 0.f) : s_gy[n][wv * LS_R + r];
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float p = lane_of(pv[r], j), tt, lt;
                        if (!bg) {
                            tt = cx[j].x * cy.x;                // einsum("BNW, BNH -> BNHW"): one fp32 product
                            mx[r][j] = fmaxf(mx[r][j], tt);
                            lt = cx[j].y + cy.y;
                        } else {
                            tt = 1.0f - mx[r][j];
                            lt = 0.f;
                        }
                        if (m != 1.0f) { p *= m; tt *= m; }      // loss.py:94-103 (wave-uniform branch: m belongs to the channel)
                        if (KL && (bg || m != 1.0f)) lt = logf(tt);
                        element<MSE, KL, AW>(p, tt, lt, s0, s1, s2);
                    }
                }
            }
            acc[0] += (double)s0; acc[1] += (double)s1; acc[2] += (double)s2;
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

// one thread per (frame, term): the partials of the frame in index order
__global__ void loss_fold_kernel(const double* __restrict__ part, int B, int per_frame, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * 3) return;
    const int b = i / 3, k = i - b * 3;
    double v = 0.0;
    for (int j = 0; j < per_frame; ++j) v += part[((size_t)b * per_frame + j) * 3 + k];
    out[i] = v;
}

template <int V>
void launch(int terms, dim3 grid, hipStream_t st, const float* logp, const float* mask, const float2* gx, const float2* gy, int N, int h, int w,
            double* part) {
#define LS_CASE(T, A, B_, C) case T: hipLaunchKernelGGL((loss_kernel<V, A, B_, C>), grid, dim3(256), 0, st, logp, mask, gx, gy, N, h, w, part); break;
    switch (terms) {
        LS_CASE(1, true, false, false) LS_CASE(2, false, true, false) LS_CASE(3, true, true, false) LS_CASE(4, false, false, true)
        LS_CASE(5, true, false, true) LS_CASE(6, false, true, true) LS_CASE(7, true, true, true)
    }
#undef LS_CASE
}

int vec_width(const float* d_logp, int w) { return (w % 4 == 0 && ((uintptr_t)d_logp & 15) == 0) ? 4 : 1; }

struct Coef3 { float c[3]; };

// d/dx of the three terms at one element, x the logit, p = x * m, t = target * m; the common factor m is applied by the caller
//   (exp(p) - t)^2          ->  2 (e - t) e
//   xlogy(t, t) - t p       ->  -t                       (0 where t = 0)
//   adaptive_wing(e, t)     ->  w'(|t - e|) sign(e - t) e
template <bool MSE, bool KL, bool AW>
__device__ __forceinline__ float grad_element(float p, float t, const Coef3& cf) {
    const float e = expf(p);
    float g = 0.f;
    if (MSE) g += cf.c[0] * (2.0f * (e - t) * e);
    if (KL) g += cf.c[1] * -t;
    if (AW) g += cf.c[2] * (sncal::adaptive_wing_grad(e, t) * e);
    return g;
}

// The tiling and the channel walk of loss_kernel; each element's gradient is stored where its logit was read.  No sums, so no
// LDS reduction and no partials: a lane's V gradients of a row go out in one store.
template <int V, bool MSE, bool KL, bool AW>
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ logp, const float* __restrict__ mask,
                                                        const float2* __restrict__ gxt, const float2* __restrict__ gyt, int N, int h, int w,
                                                        Coef3 cf, const float* __restrict__ gout, float* __restrict__ grad) {
    using VT = typename Vec<V>::type;
    __shared__ float s_gy[LS_MAXN][LS_ROWS];
    __shared__ float s_m[LS_MAXN + 1];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, b = blockIdx.z;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    for (int i = t; i < N * LS_ROWS; i += 256) {
        const int n = i / LS_ROWS, r = i - n * LS_ROWS;
        s_gy[n][r] = y0 + r < h ? gyt[((size_t)b * N + n) * h + y0 + r].x : 0.f;
    }
    for (int i = t; i <= N; i += 256) s_m[i] = mask ? mask[(size_t)b * (N + 1) + i] : 1.0f;
    __syncthreads();
    const int yw = y0 + wv * LS_R;
    const int rows = min(LS_R, h - yw);
    if (x0 >= w || rows <= 0) return;                           // w % V == 0, so a live lane owns V whole columns
    const float go = gout ? *gout : 1.0f;
    const size_t plane = (size_t)h * w, off = (size_t)b * (N + 1) * plane + (size_t)yw * w + x0;
    float mx[LS_R][V];
#pragma unroll
    for (int r = 0; r < LS_R; ++r)
#pragma unroll
        for (int j = 0; j < V; ++j) mx[r][j] = 0.f;
#pragma unroll 2
    for (int n = 0; n <= N; ++n) {
        const bool bg = n == N;
        const float m = s_m[n];
        float cx[V];
        if (!bg) {
#pragma unroll
            for (int j = 0; j < V; ++j) cx[j] = gxt[((size_t)b * N + n) * w + x0 + j].x;
        }
        VT pv[LS_R];
#pragma unroll
        for (int r = 0; r < LS_R; ++r)
            if (r < rows) pv[r] = *reinterpret_cast<const VT*>(logp + off + (size_t)n * plane + (size_t)r * w);
#pragma unroll
        for (int r = 0; r < LS_R; ++r) {
            if (r < rows) {
                const float cy = bg ? 0.f : s_gy[n][wv * LS_R + r];
                float gv[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float p = lane_of(pv[r], j), tt;
                    if (!bg) {
                        tt = cx[j] * cy;                        // the target of loss_kernel, formed the same way
                        mx[r][j] = fmaxf(mx[r][j], tt);
                    } else {
                        tt = 1.0f - mx[r][j];
                    }
                    if (m != 1.0f) { p *= m; tt *= m; }
                    float g = grad_element<MSE, KL, AW>(p, tt, cf);
                    if (m != 1.0f) g *= m;                      // d(x * m) / dx
                    gv[j] = go * g;
                }
                float* const o = grad + off + (size_t)n * plane + (size_t)r * w;
                if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                else *o = gv[0];
            }
        }
    }
}

template <int V>
void launch_grad(int terms, dim3 grid, hipStream_t st, const float* logp, const float* mask, const float2* gx, const float2* gy, int N, int h,
                 int w, Coef3 cf, const float* gout, float* grad) {
#define LS_CASE(T, A, B_, C) case T: hipLaunchKernelGGL((loss_grad_kernel<V, A, B_, C>), grid, dim3(256), 0, st, logp, mask, gx, gy, N, h, w, cf, gout, grad); break;
    switch (terms) {
        LS_CASE(1, true, false, false) LS_CASE(2, false, true, false) LS_CASE(3, true, true, false) LS_CASE(4, false, false, true)
        LS_CASE(5, true, false, true) LS_CASE(6, false, true, true) LS_CASE(7, true, true, true)
    }
#undef LS_CASE
}

}  // namespace

extern "C" int sncal_heatmap_loss_workspace(int B, int N, int h, int w, size_t* bytes) {
    SNCAL_CHECK_ARG(bytes, "sncal_heatmap_loss_workspace: null pointer");
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= LS_MAXN && h > 0 && w > 0, "sncal_heatmap_loss_workspace: B=%d N=%d h=%d w=%d (N <= %d)", B, N, h, w,
                    LS_MAXN);
    *bytes = layout(B, N, h, w, 1).total;                       // V = 1 has the most partials: enough for either width
    return SNCAL_OK;
}

extern "C" int sncal_heatmap_loss(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w, float sigma,
                                  float stride, int terms, double* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= LS_MAXN && h > 0 && w > 0, "sncal_heatmap_loss: B=%d N=%d h=%d w=%d (N <= %d)", B, N, h, w, LS_MAXN);
    SNCAL_CHECK_ARG(sigma > 0.f, "sncal_heatmap_loss: sigma %g", (double)sigma);
    SNCAL_CHECK_ARG(stride > 0.f, "sncal_heatmap_loss: stride %g", (double)stride);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 7, "sncal_heatmap_loss: terms %d (bit0 mse, bit1 kl, bit2 awing)", terms);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_logp && d_kpts && d_out, "sncal_heatmap_loss: null pointer");
    hipStream_t st = sncal::as_stream(stream);
    if (terms == 0) {
        SNCAL_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)B * 3 * sizeof(double), st));
        return SNCAL_OK;
    }
    const int V = vec_width(d_logp, w);
    const Layout L = layout(B, N, h, w, V);
    SNCAL_CHECK_ARG(B <= 65535 && L.by <= 65535 && (size_t)B * N <= 0x7fffffffu, "sncal_heatmap_loss: grid too large");
    SNCAL_CHECK_ARG(d_ws && ((uintptr_t)d_ws & 15) == 0, "sncal_heatmap_loss: workspace pointer null or not 16-byte aligned");
    if (ws_bytes < L.total) {
        sncal::set_error("sncal_heatmap_loss: workspace %zu bytes, need %zu (sncal_heatmap_loss_workspace)", ws_bytes, L.total);
        return SNCAL_ERR_WORKSPACE;
    }
    float2* const gx = reinterpret_cast<float2*>((char*)d_ws + L.gx);
    float2* const gy = reinterpret_cast<float2*>((char*)d_ws + L.gy);
    double* const part = reinterpret_cast<double*>((char*)d_ws + L.part);
    hipLaunchKernelGGL(loss_tables_kernel, dim3(B * N), dim3(256), 0, st, d_kpts, N, sigma, stride, h, w, gx, gy);
    SNCAL_CHECK_LAUNCH();
    const dim3 grid(L.bx, L.by, B);
    if (V == 4) launch<4>(terms, grid, st, d_logp, d_mask, gx, gy, N, h, w, part);
    else launch<1>(terms, grid, st, d_logp, d_mask, gx, gy, N, h, w, part);
    SNCAL_CHECK_LAUNCH();
    hipLaunchKernelGGL(loss_fold_kernel, dim3((B * 3 + 63) / 64), dim3(64), 0, st, part, B, L.bx * L.by, d_out);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_heatmap_loss_grad(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w,
                                       float sigma, float stride, int terms, const double coef[3], const float* d_gout, float* d_grad,
                                       void* d_ws, size_t ws_bytes, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= LS_MAXN && h > 0 && w > 0, "sncal_heatmap_loss_grad: B=%d N=%d h=%d w=%d (N <= %d)", B, N, h, w,
                    LS_MAXN);
    SNCAL_CHECK_ARG(sigma > 0.f, "sncal_heatmap_loss_grad: sigma %g", (double)sigma);
    SNCAL_CHECK_ARG(stride > 0.f, "sncal_heatmap_loss_grad: stride %g", (double)stride);
    SNCAL_CHECK_ARG(terms >= 0 && terms <= 7, "sncal_heatmap_loss_grad: terms %d (bit0 mse, bit1 kl, bit2 awing)", terms);
    SNCAL_CHECK_ARG(coef, "sncal_heatmap_loss_grad: null coef");
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_logp && d_kpts && d_grad, "sncal_heatmap_loss_grad: null pointer");
    hipStream_t st = sncal::as_stream(stream);
    if (terms == 0) {
        SNCAL_CHECK_HIP(hipMemsetAsync(d_grad, 0, (size_t)B * (N + 1) * h * w * sizeof(float), st));
        return SNCAL_OK;
    }
    const int V = vec_width(d_logp, w) == 4 && vec_width(d_grad, w) == 4 ? 4 : 1;
    const Layout L = layout(B, N, h, w, V);
    SNCAL_CHECK_ARG(B <= 65535 && L.by <= 65535 && (size_t)B * N <= 0x7fffffffu, "sncal_heatmap_loss_grad: grid too large");
    SNCAL_CHECK_ARG(d_ws && ((uintptr_t)d_ws & 15) == 0, "sncal_heatmap_loss_grad: workspace pointer null or not 16-byte aligned");
    if (ws_bytes < L.part) {                                    // the tables only: no partial sums here
        sncal::set_error("sncal_heatmap_loss_grad: workspace %zu bytes, need %zu (sncal_heatmap_loss_workspace covers it)", ws_bytes, L.part);
        return SNCAL_ERR_WORKSPACE;
    }
    float2* const gx = reinterpret_cast<float2*>((char*)d_ws + L.gx);
    float2* const gy = reinterpret_cast<float2*>((char*)d_ws + L.gy);
    const Coef3 cf = {{(float)coef[0], (float)coef[1], (float)coef[2]}};
    hipLaunchKernelGGL(loss_tables_kernel, dim3(B * N), dim3(256), 0, st, d_kpts, N, sigma, stride, h, w, gx, gy);
    SNCAL_CHECK_LAUNCH();
    const dim3 grid(L.bx, L.by, B);
    if (V == 4) launch_grad<4>(terms, grid, st, d_logp, d_mask, gx, gy, N, h, w, cf, d_gout, d_grad);
    else launch_grad<1>(terms, grid, st, d_logp, d_mask, gx, gy, N, h, w, cf, d_gout, d_grad);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
