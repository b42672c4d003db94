// The frame of the four fused streaming loss kernels (loss.hip: loss_kernel, loss_grad_kernel; line_loss.hip: line_loss_kernel,
// line_grad_kernel): the tiling, the channel walk, the LDS staging, the fixed-order reduction and fold, the workspace layout, the
// dispatch to an instantiation and the host prologue -- each written once.  The two .hip files keep what is theirs: the tables
// kernels and the per-element arithmetic of their terms (and loss.hip one sums kernel written out, for the reason given there).
// Tiling: a workgroup of LS_WAVES = 4 waves owns LS_ROWS = 16 rows x 64 * V columns of one frame; a wave owns LS_R = 4 of the
// rows, a lane V consecutive columns of them (V = 4: 16-byte loads and stores, when w % 4 == 0 and every base is 16-byte aligned;
// V = 1 otherwise).  Row factors of the target live in LDS, column factors in registers; the channel loop is unrolled by 2.
//   loss_walk<V>(pred, C, h, w, model, sink)
// A MODEL says what a channel's target is: stage() fills LDS (and holds the barrier), channel() / row() fetch the factors,
// load_row() issues loads that go beside the prediction's, target() forms one element's target (and may scale the prediction),
// chain() applies d(prediction as the terms see it) / d(prediction in memory).  A SINK says what happens to each element: SumSink
// adds K terms up, StoreSink writes the gradient.  Both take the arithmetic of the terms from the includer (`Terms`: sum() or
// grad()).  Plain structs, everything inlined: the kernels hold no call.
// Sums and gradient of one model form the target in the same code, hence with the same bits: the bitwise tests rely on it.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "common.hpp"

namespace sncal {

constexpr int LS_MAXC = 64, LS_R = 4, LS_WAVES = 4, LS_ROWS = LS_R * LS_WAVES;

template <int V> struct Vec;
template <> struct Vec<4> { using type = float4; };
template <> struct Vec<1> { using type = float; };
__device__ __forceinline__ float lane_of(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ float lane_of(const float& v, int) { return v; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- the thread's position ------------------------------------------------------------------------------------------------------
struct LossTile { int lane, wv, b, y0, x0, yw, rows; bool live; };
template <int V>
__device__ __forceinline__ LossTile loss_tile(int h, int w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int y0 = blockIdx.y * LS_ROWS, x0 = (blockIdx.x * 64 + lane) * V;
    const int yw = y0 + wv * LS_R;                              // first row of this wave
    const int rows = min(LS_R, h - yw);                         // <= 0: the wave has no row (it still joins the barriers)
    return {lane, wv, (int)blockIdx.z, y0, x0, yw, rows, x0 < w && rows > 0};      // w % V == 0, so a live lane owns V whole columns
}

// a table cell as the kernel keeps it: float2 {Gaussian, its exp argument}, or the Gaussian alone
template <class T> __device__ __forceinline__ T cell(const float2& v) { if constexpr (std::is_same<T, float2>::value) return v; else return v.x; }
template <class T> __device__ __forceinline__ T cell(float v) { return v; }
__device__ __forceinline__ float gauss_of(const float2& v) { return v.x; }
__device__ __forceinline__ float gauss_of(float v) { return v; }

// rows y0 .. y0 + LS_ROWS - 1 of the G row tables (h cells each) of frame tl.b -> LDS, zero below the map; no barrier
template <class T, class S>
__device__ __forceinline__ void stage_rows(T (*dst)[LS_ROWS], const S* __restrict__ table, int G, const LossTile& tl, int h) {
    for (int i = threadIdx.x; i < G * LS_ROWS; i += 256) {
        const int g = i / LS_ROWS, r = i - g * LS_ROWS;
        dst[g][r] = tl.y0 + r < h ? cell<T>(table[((size_t)tl.b * G + g) * h + tl.y0 + r]) : T{};
    }
}

// ---- models ---------------------------------------------------------------------------------------------------------------------
// Keypoint heatmaps (loss.hip): N Gaussian channels gx[n][x] * gy[n][y] from the float2 tables, then the background channel
// 1 - running max; p and t times the channel's mask (loss.py:94-103; a wave-uniform branch: m belongs to the channel).  LOG: the
// sink wants log t -- analytic (the sum of the two exp arguments) on keypoint channels with mask 1, logf elsewhere; without it
// the tables' arguments are dropped on load and the LDS rows are float.
template <int V, bool LOG>
struct KeypointModel {
    using T = typename std::conditional<LOG, float2, float>::type;
    const float* mask;
    const float2 *gxt, *gyt;
    int N;
    T cx[V], cy;
    float mx[LS_R][V], m;
    bool bg;
    static __device__ __forceinline__ T (&s_gy())[LS_MAXC][LS_ROWS] { __shared__ T s[LS_MAXC][LS_ROWS]; return s; }
    static __device__ __forceinline__ float (&s_m())[LS_MAXC + 1] { __shared__ float s[LS_MAXC + 1]; return s; }

    __device__ __forceinline__ void stage(const LossTile& tl, int h) {
        stage_rows(s_gy(), gyt, N, tl, h);
        for (int i = threadIdx.x; i <= N; i += 256) s_m()[i] = mask ? mask[(size_t)tl.b * (N + 1) + i] : 1.0f;
        __syncthreads();
    }
    __device__ __forceinline__ void begin() {
#pragma unroll
        for (int r = 0; r < LS_R; ++r)
#pragma unroll
            for (int j = 0; j < V; ++j) mx[r][j] = 0.f;         // targets are >= 0 and N >= 1: the same max as torch.max over the channels
    }
    __device__ __forceinline__ void channel(const LossTile& tl, int n, int w) {
        bg = n == N;
        m = s_m()[n];
        if (!bg) {
#pragma unroll
            for (int j = 0; j < V; ++j) cx[j] = cell<T>(gxt[((size_t)tl.b * N + n) * w + tl.x0 + j]);
        }
    }
    __device__ __forceinline__ void load_row(int, size_t) {}
    __device__ __forceinline__ void row(const LossTile& tl, int n, int r) { cy = bg ? cell<T>(make_float2(0.f, 0.f)) : s_gy()[n][tl.wv * LS_R + r]; }
    __device__ __forceinline__ float target(int r, int j, float& p, float& logt) {
        float t;
        if (!bg) {
            t = gauss_of(cx[j]) * gauss_of(cy);                 // einsum("BNW, BNH -> BNHW"): one fp32 product
            mx[r][j] = fmaxf(mx[r][j], t);
            if constexpr (LOG) logt = cx[j].y + cy.y;
        } else {
            t = 1.0f - mx[r][j];
            logt = 0.f;
        }
        if (m != 1.0f) { p *= m; t *= m; }
        if (LOG && (bg || m != 1.0f)) logt = logf(t);
        return t;
    }
    __device__ __forceinline__ float chain(float g) const { return m != 1.0f ? g * m : g; }       // d(x * m) / dx
};

// keypoint_map += gauss, first point first (0 + a is a): line_target_kernel and the rebuild model form an element in this one place
__device__ __forceinline__ float line_target_value(float gx0, float gy0, float gx1, float gy1) {
    float t = gx0 * gy0;
    t = t + gx1 * gy1;
    return t;
}

// Line maps rebuilt from the endpoints (line_loss.hip): two factors per axis, gx (B*C, 2, w) and gy (B*C, 2, h)
template <int V>
struct LineRebuildModel {
    using VT = typename Vec<V>::type;
    const float *gxt, *gyt;
    int C;
    VT cx0, cx1;
    float cy0, cy1;
    static __device__ __forceinline__ float (&s_gy())[2 * LS_MAXC][LS_ROWS] { __shared__ float s[2 * LS_MAXC][LS_ROWS]; return s; }

    __device__ __forceinline__ void stage(const LossTile& tl, int h) {
        stage_rows(s_gy(), gyt, 2 * C, tl, h);
        __syncthreads();
    }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void channel(const LossTile& tl, int c, int w) {
        cx0 = *reinterpret_cast<const VT*>(gxt + ((size_t)tl.b * C + c) * 2 * w + tl.x0);
        cx1 = *reinterpret_cast<const VT*>(gxt + (((size_t)tl.b * C + c) * 2 + 1) * w + tl.x0);
    }
    __device__ __forceinline__ void load_row(int, size_t) {}
    __device__ __forceinline__ void row(const LossTile& tl, int c, int r) {
        cy0 = s_gy()[2 * c][tl.wv * LS_R + r];
        cy1 = s_gy()[2 * c + 1][tl.wv * LS_R + r];
    }
    __device__ __forceinline__ float target(int, int j, float&, float&) const { return line_target_value(lane_of(cx0, j), cy0, lane_of(cx1, j), cy1); }
    __device__ __forceinline__ float chain(float g) const { return g; }
};

// Line maps as a loader delivers them: the target is read from memory beside the prediction.  No table, no LDS, no barrier.
template <int V>
struct LineMapsModel {
    using VT = typename Vec<V>::type;
    const float* maps;
    VT tv[LS_R];
    __device__ __forceinline__ void stage(const LossTile&, int) {}
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void channel(const LossTile&, int, int) {}
    __device__ __forceinline__ void load_row(int r, size_t at) { tv[r] = *reinterpret_cast<const VT*>(maps + at); }
    __device__ __forceinline__ void row(const LossTile&, int, int) {}
    __device__ __forceinline__ float target(int r, int j, float&, float&) const { return lane_of(tv[r], j); }
    __device__ __forceinline__ float chain(float g) const { return g; }
};

// ---- sinks ----------------------------------------------------------------------------------------------------------------------
// K sums per frame.  The order is fixed: a channel's LS_R * V elements in fp32, rows then columns; one fp64 add per channel and
// lane; wave shuffle -> LDS -> the 4 waves in index order -> one partial per workgroup.  No atomics: two runs give the same bits.
template <class Terms>
struct SumSink {
    static constexpr int K = Terms::K;
    Terms terms;
    double* part;
    double acc[K] = {};
    float s[K];
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void channel_begin() {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] = 0.f;
    }
    template <class Model>
    __device__ __forceinline__ void element(const Model&, int, float p, float t, float logt) { terms.sum(p, t, logt, s); }
    __device__ __forceinline__ void row_end(size_t) {}
    __device__ __forceinline__ void channel_end() {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += (double)s[k];
    }
    __device__ __forceinline__ void finish(const LossTile& tl) {      // every wave comes here, with or without rows
        __shared__ double s_red[LS_WAVES][K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double v = wave_sum(acc[k]);
            if (tl.lane == 0) s_red[tl.wv][k] = v;
        }
        __syncthreads();
        const int t = threadIdx.x;
        if (t < K) {
            double v = 0.0;
            for (int i = 0; i < LS_WAVES; ++i) v += s_red[i][t];
            part[(((size_t)tl.b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * K + t] = v;
        }
    }
};

// one thread per (frame, term): the partials of the frame in index order
template <int K>
__global__ void loss_fold_kernel(const double* __restrict__ part, int B, int per_frame, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K, k = i - b * K;
    double v = 0.0;
    for (int j = 0; j < per_frame; ++j) v += part[((size_t)b * per_frame + j) * K + k];
    out[i] = v;
}

// The gradient, stored where the prediction was read: gout * chain(sum_k coef_k * term_k') in fp32, gout a device scalar
// (NULL = 1) read once per lane; a lane's V gradients of a row go out in one store.  No sums, so no reduction and no partials.
template <int V, class Terms>
struct StoreSink {
    Terms terms;
    const float* gout;
    float* grad;
    float go, gv[V];
    __device__ __forceinline__ void begin() { go = gout ? *gout : 1.0f; }
    __device__ __forceinline__ void channel_begin() {}
    template <class Model>
    __device__ __forceinline__ void element(const Model& M, int j, float p, float t, float) { gv[j] = go * M.chain(terms.grad(p, t)); }
    __device__ __forceinline__ void row_end(size_t at) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(grad + at) = make_float4(gv[0], gv[1], gv[2], gv[3]);
        else grad[at] = gv[0];
    }
    __device__ __forceinline__ void channel_end() {}
    __device__ __forceinline__ void finish(const LossTile&) {}
};

// ---- the walk -------------------------------------------------------------------------------------------------------------------
// pred (B, C, h, w): every element of the workgroup's tile once, channel by channel
template <int V, class Model, class Sink>
__device__ __forceinline__ void loss_walk(const float* __restrict__ pred, int C, int h, int w, Model& M, Sink& S) {
    using VT = typename Vec<V>::type;
    const LossTile tl = loss_tile<V>(h, w);
    M.stage(tl, h);
    if (tl.live) {
        const size_t plane = (size_t)h * w, off = (size_t)tl.b * C * plane + (size_t)tl.yw * w + tl.x0;
        S.begin();
        M.begin();
#pragma unroll 2
        for (int c = 0; c < C; ++c) {
            M.channel(tl, c, w);
            VT pv[LS_R];
#pragma unroll
            for (int r = 0; r < LS_R; ++r)
                if (r < tl.rows) {
                    const size_t at = off + (size_t)c * plane + (size_t)r * w;
                    pv[r] = *reinterpret_cast<const VT*>(pred + at);
                    M.load_row(r, at);
                }
            S.channel_begin();
#pragma unroll
            for (int r = 0; r < LS_R; ++r) {
                if (r < tl.rows) {
                    M.row(tl, c, r);
#pragma unroll
                    for (int j = 0; j < V; ++j) {
                        float p = lane_of(pv[r], j), logt = 0.f;
                        const float t = M.target(r, j, p, logt);
                        S.element(M, j, p, t, logt);
                    }
                    S.row_end(off + (size_t)c * plane + (size_t)r * w);
                }
            }
            S.channel_end();
        }
    }
    S.finish(tl);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
// terms (1 .. T) and V (4 or 1) -> f(integral_constant<int, terms>, integral_constant<int, V>): the instantiation to launch
template <int T, class F>
void loss_dispatch(int terms, int V, F&& f) {
    if constexpr (T > 0) {
        if (terms != T) return loss_dispatch<T - 1>(terms, V, f);
        if (V == 4) f(std::integral_constant<int, T>{}, std::integral_constant<int, 4>{});
        else f(std::integral_constant<int, T>{}, std::integral_constant<int, 1>{});
    }
}

inline bool aligned16(std::initializer_list<const void*> ps) {   // a null pointer (an absent tensor) does not narrow anything
    for (const void* p : ps) if ((uintptr_t)p & 15) return false;
    return true;
}

// B frames of C table channels on an h x w map; `cell` = bytes of the tables per (frame, channel, axis cell), K = sums per frame
struct LossShape { int B, C, h, w; size_t cell; int K; };
// workspace: column tables | row tables | K partials per workgroup (256-byte aligned parts); bx, by = workgroups per frame
struct LossLayout { size_t gx, gy, part, total; int bx, by; };
inline LossLayout loss_layout(const LossShape& s, int V) {
    LossLayout L;
    L.bx = (s.w + 64 * V - 1) / (64 * V);
    L.by = (s.h + LS_ROWS - 1) / LS_ROWS;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.gx = 0;
    L.gy = up((size_t)s.B * s.C * s.w * s.cell);
    L.part = L.gy + up((size_t)s.B * s.C * s.h * s.cell);
    L.total = L.part + up((size_t)s.B * L.bx * L.by * s.K * sizeof(double));
    return L;
}
inline size_t loss_workspace_bytes(const LossShape& s) { return loss_layout(s, 1).total; }   // V = 1 has the most partials: enough for either width

// What the four entry points do between their own argument checks (shape, terms, B == 0, pointers) and their launches.  `fn` is
// the function the caller called: every message starts with it.  terms == 0: `out` is zeroed and `done` set, before the workspace
// is looked at.  Otherwise V from the width and `aligned`, the grid, and the workspace as far as `need` says: LOSS_WS_ALL (sums),
// LOSS_WS_TABLES (a gradient that rebuilds the target) or LOSS_WS_NONE (a gradient on maps), checked and carved.
enum LossWs { LOSS_WS_NONE, LOSS_WS_TABLES, LOSS_WS_ALL };
struct LossLaunch { hipStream_t st; bool done; int V, per_frame; dim3 grid; void *gx, *gy; double* part; };
inline int loss_prologue(LossLaunch& L, const char* fn, const char* ws_fn, const LossShape& s, int terms, void* out, size_t out_bytes,
                         bool aligned, LossWs need, void* d_ws, size_t ws_bytes, void* stream) {
    L = LossLaunch{};
    L.st = as_stream(stream);
    L.done = terms == 0;
    if (L.done) {
        SNCAL_CHECK_HIP(hipMemsetAsync(out, 0, out_bytes, L.st));
        return SNCAL_OK;
    }
    L.V = (s.w % 4 == 0 && aligned) ? 4 : 1;
    const LossLayout lay = loss_layout(s, L.V);
    SNCAL_CHECK_ARG(s.B <= 65535 && lay.by <= 65535 && (size_t)s.B * s.C <= 0x7fffffffu, "%s: grid too large", fn);
    L.grid = dim3(lay.bx, lay.by, s.B);
    L.per_frame = lay.bx * lay.by;
    if (need == LOSS_WS_NONE) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_ws && aligned16({d_ws}), "%s: workspace pointer null or not 16-byte aligned", fn);
    const size_t bytes = need == LOSS_WS_ALL ? lay.total : lay.part;      // the tables only: a gradient has no partial sums
    if (ws_bytes < bytes) {
        set_error("%s: workspace %zu bytes, need %zu (%s%s)", fn, ws_bytes, bytes, ws_fn, need == LOSS_WS_ALL ? "" : " covers it");
        return SNCAL_ERR_WORKSPACE;
    }
    L.gx = (char*)d_ws + lay.gx;
    L.gy = (char*)d_ws + lay.gy;
    L.part = reinterpret_cast<double*>((char*)d_ws + lay.part);
    return SNCAL_OK;
}

}  // namespace sncal
