// The dev-kit's extremity metric on the device: per-frame tp / fp / fn of detected line ends against the annotation, a batch and
// up to eight pixel thresholds in one launch.
//   /root/reference/baseline/evaluate_extremities.py:37-116   evaluate_detection_prediction (extremities.py restates it on the host)
//   /root/reference/baseline/evaluate_extremities.py:119-134  scale_points: normalised -> pixels by (W - 1, H - 1)
//   /root/reference/baseline/evaluate_extremities.py:192-216  both labellings per frame, the better accuracy kept, a tie is mirrored
//   /root/reference/src/utils/export_line_result.py:115-124   get_line_data's `points`: the peaks form of the prediction
// One workgroup of one wavefront per frame.  Lane l * 32 + c holds class c (ANNOT_CLASSES order) under labelling l: the prediction's
// class c against the annotation's class c (l = 0) or EX_SYM[c] (l = 1).  A lane reads the first and last point of its two classes
// where they lie, so a frame's state is registers: no LDS, no workspace.  The counts of a labelling are sums over its half of the
// wave (integers: exact, order-free); lane 0 takes the reference's decision per threshold and the class lanes of the chosen half
// store their rows.  fp64 without contraction; the accuracies are float32 quotients as the reference's float32 confusion matrix
// gives them.  Plain stores, no atomics: two runs write the same bits.
#include "common.hpp"
#include "../../include/sncal.h"
#include <cmath>

namespace {

constexpr int EX_NCLS = 28, EX_FIRST_LINE = 3, EX_MAX_PEAK_C = 23, EX_MAXT = 8;
constexpr int EX_CENTRAL = 0;                               // 'Circle central': removed from both sides (:58-61)
// SoccerPitch.symetric_classes in ANNOT_CLASSES ids (tests/test_extremities_host.py compares it with evaluate.SYMMETRIC)
__constant__ unsigned char EX_SYM[EX_NCLS] = {0, 2, 1, 8, 17, 5, 11, 19, 3, 22, 20, 6, 15, 25, 18, 12, 23, 4, 14, 7, 10, 24, 9, 16, 21, 13, 26, 27};

struct ExTs { double t[EX_MAXT]; };

// a class of one side: n points, the first and the last in pixels
struct Ends {
    int n;
    double ax, ay, bx, by;
};

// scale_points on a packed class: a range that leaves [0, total] reads as empty
__device__ inline Ends packed_ends(const double* __restrict__ pts, int total, const int* __restrict__ off, int c, double sx, double sy) {
    Ends e = {0, 0.0, 0.0, 0.0, 0.0};
    const int lo = off[c], hi = off[c + 1];
    if (lo < 0 || hi <= lo || hi > total) return e;
    e.n = hi - lo;
    const double* a = pts + 2 * (size_t)lo;
    const double* b = pts + 2 * (size_t)(hi - 1);
    e.ax = a[0] * sx; e.ay = a[1] * sy;
    e.bx = b[0] * sx; e.by = b[1] * sy;
    return e;
}

// get_line_data's points of channel k: the slots with p >= p_threshold, in slot order, (x * scale, y * scale) in fp32
__device__ inline Ends peak_ends(const float* __restrict__ rows, float scale, float p_threshold) {
    Ends e = {0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float x = rows[3 * i], y = rows[3 * i + 1], p = rows[3 * i + 2];
        if (!(p >= p_threshold)) continue;
        const double px = (double)(x * scale), py = (double)(y * scale);
        if (e.n == 0) { e.ax = px; e.ay = py; }
        e.bx = px; e.by = py;
        ++e.n;
    }
    return e;
}

// distance(): sqrt of the two squares summed in (x, y) order
__device__ inline double dist(double ax, double ay, double bx, double by) {
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

// sum over the lane's half of the wave (lanes 0..31 / 32..63), in every lane of it
__device__ inline int half_sum(int v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// confusion[0, 0] / confusion.sum() on the float32 matrix; 0 when it is empty (:200-205)
__device__ inline float accuracy(int tp, int fp, int fn) {
    const float s = (float)tp + (float)fp + (float)fn;
    return s > 0.f ? (float)((double)(float)tp / (double)s) : 0.f;         // the correctly rounded float32 quotient
}

__global__ __launch_bounds__(64) void extremity_counts_kernel(const double* __restrict__ gt_pts, int gt_total, const int* __restrict__ gt_off,
                                                              const float* __restrict__ peaks, int C, float scale, float p_threshold,
                                                              const double* __restrict__ pr_pts, int pr_total, const int* __restrict__ pr_off,
                                                              int B, int img_w, int img_h, ExTs ts, int n_t, int* __restrict__ d_frame,
                                                              int* __restrict__ d_class, double* __restrict__ d_err) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int l = lane >> 5, c = lane & 31;
    const bool cls = c < EX_NCLS;
    const bool scored = cls && c != EX_CENTRAL;
    const double sx = (double)(img_w - 1), sy = (double)(img_h - 1);
    Ends pr = {0, 0.0, 0.0, 0.0, 0.0}, gt = {0, 0.0, 0.0, 0.0, 0.0};
    if (scored) {
        if (peaks) {
            const int k = c - EX_FIRST_LINE;
            if (k >= 0 && k < C) pr = peak_ends(peaks + ((size_t)b * C + k) * 6, scale, p_threshold);
        } else {
            pr = packed_ends(pr_pts, pr_total, pr_off + (size_t)b * (EX_NCLS + 1), c, sx, sy);
        }
        gt = packed_ends(gt_pts, gt_total, gt_off + (size_t)b * (EX_NCLS + 1), l ? (int)EX_SYM[c] : c, sx, sy);
    }
    const bool both = pr.n > 0 && gt.n > 0;
    double d1 = NAN, d2 = NAN;
    if (both) {
        d1 = dist(gt.ax, gt.ay, pr.ax, pr.ay);
        const double d1rev = dist(gt.bx, gt.by, pr.ax, pr.ay);
        d2 = dist(gt.bx, gt.by, pr.bx, pr.by);
        const double d2rev = dist(gt.ax, gt.ay, pr.bx, pr.by);
        if (d1rev <= d1 && d2rev <= d2) { d1 = d1rev; d2 = d2rev; }
    }
    for (int it = 0; it < n_t; ++it) {
        const double t = ts.t[it];
        int tp = 0, fp = 0, fn = 0;
        if (both) {
            tp = (d1 < t ? 1 : 0) + (d2 < t ? 1 : 0);
            fp = 2 - tp;                                       // too far: a false positive (:102-114)
        } else {
            fp = pr.n;                                         // only detected (:63-67)
            fn = gt.n;                                         // only annotated (:69-73)
        }
        const int my_tp = half_sum(tp), my_fp = half_sum(fp), my_fn = half_sum(fn);
        const int ot_tp = __shfl_xor(my_tp, 32, 64), ot_fp = __shfl_xor(my_fp, 32, 64), ot_fn = __shfl_xor(my_fn, 32, 64);
        int choice = 0;
        if (lane == 0) choice = accuracy(my_tp, my_fp, my_fn) > accuracy(ot_tp, ot_fp, ot_fn) ? 0 : 1;      // a tie is mirrored (:207-216)
        choice = __shfl(choice, 0, 64);
        const size_t fr = (size_t)it * B + b;
        if (lane == 0) {
            int* f = d_frame + fr * 4;
            f[0] = choice ? ot_tp : my_tp;
            f[1] = choice ? ot_fp : my_fp;
            f[2] = choice ? ot_fn : my_fn;
            f[3] = choice;
        }
        if (cls && l == choice) {
            int* r = d_class + (fr * EX_NCLS + c) * 3;
            r[0] = tp; r[1] = fp; r[2] = fn;
            double* e = d_err + (fr * EX_NCLS + c) * 2;
            e[0] = d1; e[1] = d2;
        }
    }
}

}  // namespace

extern "C" int sncal_extremity_counts(const double* d_gt_points, int total_points, const int* d_gt_offsets, const float* d_peaks, int C,
                                      float scale, float p_threshold, const double* d_pred_points, int pred_total,
                                      const int* d_pred_offsets, int B, int n_classes, int img_w, int img_h, const double* ts, int n_t,
                                      int* d_frame, int* d_class, double* d_err, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && total_points >= 0 && pred_total >= 0, "sncal_extremity_counts: B=%d total_points=%d pred_total=%d", B,
                    total_points, pred_total);
    SNCAL_CHECK_ARG(n_classes == EX_NCLS, "sncal_extremity_counts: n_classes=%d, the class order has %d", n_classes, EX_NCLS);
    SNCAL_CHECK_ARG(n_t > 0 && n_t <= EX_MAXT, "sncal_extremity_counts: n_t %d (1..%d thresholds)", n_t, EX_MAXT);
    SNCAL_CHECK_ARG(img_w >= 1 && img_h >= 1, "sncal_extremity_counts: image %d x %d", img_w, img_h);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(!d_peaks != !(d_pred_points || d_pred_offsets),
                    "sncal_extremity_counts: exactly one of d_peaks and d_pred_points / d_pred_offsets must be given");
    SNCAL_CHECK_ARG(!d_peaks || (C >= 1 && C <= EX_MAX_PEAK_C), "sncal_extremity_counts: C=%d (1..%d line channels)", C, EX_MAX_PEAK_C);
    SNCAL_CHECK_ARG(ts && d_gt_offsets && d_frame && d_class && d_err, "sncal_extremity_counts: null pointer");
    SNCAL_CHECK_ARG(d_gt_points || total_points == 0, "sncal_extremity_counts: null ground-truth points");
    SNCAL_CHECK_ARG(d_peaks || (d_pred_offsets && (d_pred_points || pred_total == 0)), "sncal_extremity_counts: null prediction points / offsets");
    ExTs a;
    for (int k = 0; k < EX_MAXT; ++k) a.t[k] = k < n_t ? ts[k] : 0.0;
    hipLaunchKernelGGL(extremity_counts_kernel, dim3(B), dim3(64), 0, sncal::as_stream(stream), d_gt_points, total_points, d_gt_offsets,
                       d_peaks, C, scale, p_threshold, d_pred_points, pred_total, d_pred_offsets, B, img_w, img_h, a, n_t, d_frame,
                       d_class, d_err);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
