// Keypoint labels on the device: SoccerNet line / circle annotations -> the 57 keypoint labels, a batch in one launch.
//   /root/reference/src/datatools/intersections.py:53-124, ellipse.py:275-516  (annotations.get_intersections restates them)
//   /root/reference/src/models/hrnet/dataset.py:73-87                          (validate.annot_to_keypoints: the rows and the mask)
//   /root/reference/src/models/hrnet/transforms.py:136-186                     (augment.FixLRAmbiguous.decide, with LABELS_FIX_LR)
// annotations.py is the specification: every stage below restates one of its functions with the same decisions, quirks included,
// in fp64 without contraction.  What differs is the order of a few sums and the two eigen-problems (the ellipse's 3x3 by its
// characteristic cubic, the final homography by Jacobi on the 9x9 normal matrix where the host calls LAPACK), i.e. rounding.
//
// One workgroup of one wavefront per frame; the stages are separated by barriers and share the frame's labels in LDS:
//   1. lines      lane i < 30 owns LINE_INTERSECTIONS[i] and walks its two polylines in global memory (any length)
//   2. circles    lane c < 3 owns a circle: Halir-Flusser fit, tangent points, circle x line, pick_side
//   3. homography known points gathered in the host dict's order and rounded to fp32; hypotheses lane-parallel over the host's
//                 sample table (200 of them, or the one of n == 4); best = most inliers, lowest index on ties; the final fit is the
//                 unit-norm normalised DLT on the inliers: normal matrix by wave sums, smallest eigenvector by cyclic Jacobi
//   4. fill, the final inside(), the fp32 rows and the mask
// With LABELS_FIX_LR the four stages run at margin 0, lane 0 takes FixLRAmbiguous' decision from the labels, and a swapped frame (or
// any frame when the caller's margin is not 0) runs them again with the class ids permuted and the caller's margin.
// Plain stores, no atomics: two runs write the same bits.
#include "common.hpp"
#include <cstdint>
#include <cmath>

typedef unsigned long long u64;
#include "solve_wave.hpp"
#include "solve_linalg.hpp"
#include "solve_homography.hpp"

namespace {

#include "labels_tables.inc"

constexpr int NKP = 57;
constexpr int MAX_KNOWN = 53;             // ground-plane keypoints
constexpr int RANSAC_ITERS = 200;
constexpr unsigned FLAG_FIX_LR = 1u;

struct Frame {
    const double* pts;                    // the batch's points
    const int* off;                       // this frame's LB_NCLS + 1 offsets
    int total;                            // points in the batch: a class whose offsets leave [0, total] reads as empty
    unsigned present;                     // classes that are keys of the annotation
    bool swap;                            // read class c from LB_PERM[c]: flip_annot_names(swap_top_bottom=False, swap_posts=False)
    double W, H;
};

// a polyline in pixels: a class of the frame, or the two points the refinement keeps
struct Poly {
    const double* p;
    int n;
    double W, H;
    bool pair;
    double ax, ay, bx, by;
    __device__ double x(int i) const { return pair ? (i == 0 ? ax : bx) : p[2 * i] * W; }
    __device__ double y(int i) const { return pair ? (i == 0 ? ay : by) : p[2 * i + 1] * H; }
};

__device__ inline int cls_src(const Frame& f, int c) { return f.swap ? (int)LB_PERM[c] : c; }
__device__ inline bool cls_key(const Frame& f, int c) { return (f.present >> cls_src(f, c)) & 1u; }
__device__ inline Poly cls_poly(const Frame& f, int c) {
    const int s = cls_src(f, c);
    Poly l;
    l.p = f.pts + 2 * (size_t)max(f.off[s], 0);
    const int lo = f.off[s], hi = f.off[s + 1];
    l.n = cls_key(f, c) && lo >= 0 && hi >= lo && hi <= f.total ? hi - lo : 0;
    l.W = f.W; l.H = f.H; l.pair = false;
    l.ax = l.ay = l.bx = l.by = 0.0;
    return l;
}
__device__ inline Poly pair_poly(double ax, double ay, double bx, double by) {
    Poly l;
    l.p = nullptr; l.n = 2; l.W = l.H = 1.0; l.pair = true;
    l.ax = ax; l.ay = ay; l.bx = bx; l.by = by;
    return l;
}

// ---- lines -------------------------------------------------------------------------------------------------------
__device__ double mean_x(const Poly& l) {
    double s = 0.0;
    for (int i = 0; i < l.n; ++i) s += l.x(i);
    return s / (double)l.n;
}
__device__ bool is_vertical(const Poly& l, double ref) {
    const double tol = 0.5 + 1e-5 * fabs(ref);
    for (int i = 0; i < l.n; ++i)
        if (!(fabs(l.x(i) - ref) <= tol)) return false;
    return true;
}
__device__ void fit_slope(const Poly& l, double& k, double& h) {
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < l.n; ++i) { sx += l.x(i); sy += l.y(i); }
    const double xm = sx / (double)l.n, ym = sy / (double)l.n;
    double sxx = 0.0, sxy = 0.0;
    for (int i = 0; i < l.n; ++i) {
        const double dx = l.x(i) - xm;
        sxx += dx * dx;
        sxy += dx * (l.y(i) - ym);
    }
    k = sxy / sxx;
    h = ym - k * xm;
}
// two_nearest(any_side=True): the nearest and the second nearest point, ties to the lower index (the stable argsort); distances
// that do not compare (NaN) come last in index order
__device__ Poly two_nearest_any(const Poly& l, double x, double y) {
    int i0 = -1, i1 = -1;
    double d0 = INFINITY, d1 = INFINITY;
    for (int i = 0; i < l.n; ++i) {
        const double d = hypot(l.x(i) - x, l.y(i) - y);
        if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = i; }
        else if (d < d1) { d1 = d; i1 = i; }
    }
    if (i0 < 0) { i0 = 0; i1 = 1; }
    else if (i1 < 0) i1 = i0 == 0 ? 1 : 0;
    return pair_poly(l.x(i0), l.y(i0), l.x(i1), l.y(i1));
}
// two_nearest(any_side=False): the nearest point and the nearest other one whose bounding box with it holds (x, y)
__device__ bool two_nearest_bracket(const Poly& l, double x, double y, Poly& out) {
    int i0 = -1;
    double d0 = INFINITY;
    for (int i = 0; i < l.n; ++i) {
        const double d = hypot(l.x(i) - x, l.y(i) - y);
        if (d < d0) { d0 = d; i0 = i; }
    }
    if (i0 < 0) i0 = 0;
    const double fx = l.x(i0), fy = l.y(i0);
    int j0 = -1;
    double e0 = INFINITY;
    bool have = false;
    for (int j = 0; j < l.n; ++j) {
        if (j == i0) continue;
        const double px = l.x(j), py = l.y(j);
        const double lox = fmin(fx, px), hix = fmax(fx, px), loy = fmin(fy, py), hiy = fmax(fy, py);
        if (!(lox <= x && x <= hix && loy <= y && y <= hiy)) continue;
        const double d = hypot(px - x, py - y);
        if (!have || d < e0) { have = true; e0 = d; j0 = j; }
    }
    if (!have) return false;
    out = pair_poly(fx, fy, l.x(j0), l.y(j0));
    return true;
}

__device__ bool line_intersection(Poly l1, Poly l2, double& x, double& y) {
    const double eps = 1e-18;
    while (true) {
        const double m1 = mean_x(l1), m2 = mean_x(l2);
        const bool v1 = is_vertical(l1, m1), v2 = is_vertical(l2, m2);
        if (v1 && v2) return false;
        double k, h;
        if (v1) {
            x = m1;
            fit_slope(l2, k, h);
            y = k * x + h;
        } else if (v2) {
            x = m2;
            fit_slope(l1, k, h);
            y = k * x + h;
        } else {
            double k2, h2;
            fit_slope(l1, k, h);
            fit_slope(l2, k2, h2);
            x = (h2 - h) / (k - k2 + eps);
            y = k * x + h;
        }
        if (l1.n <= 2 && l2.n <= 2) return true;
        l1 = two_nearest_any(l1, x, y);
        l2 = two_nearest_any(l2, x, y);
    }
}

__device__ inline bool inside(double x, double y, double W, double H, bool within, double margin) {
    if (!within) return true;
    return -margin <= x && x <= W + margin && -margin <= y && y <= H + margin;
}

// ---- conics ------------------------------------------------------------------------------------------------------
// solve S X = R for the three columns of R (row-major 3x3 each) by elimination with partial pivoting; false when a pivot is 0
__device__ bool solve33(const double* S, const double* R, double* X) {
    double a[3][6];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { a[i][j] = S[i * 3 + j]; a[i][3 + j] = R[i * 3 + j]; }
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        for (int r = c + 1; r < 3; ++r)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (!(fabs(a[piv][c]) > 0.0)) return false;
        if (piv != c)
            for (int j = 0; j < 6; ++j) { const double t = a[c][j]; a[c][j] = a[piv][j]; a[piv][j] = t; }
        for (int r = c + 1; r < 3; ++r) {
            const double f = a[r][c] / a[c][c];
            for (int j = c; j < 6; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int j = 0; j < 3; ++j)
        for (int i = 2; i >= 0; --i) {
            double s = a[i][3 + j];
            for (int k = i + 1; k < 3; ++k) s -= a[i][k] * X[k * 3 + j];
            X[i * 3 + j] = s / a[i][i];
        }
    return true;
}

__device__ inline double det_shift(const double* A, double lam) {
    const double B[9] = {A[0] - lam, A[1], A[2], A[3], A[4] - lam, A[5], A[6], A[7], A[8] - lam};
    return det3(B);
}

// fit_ellipse: q = (a, b, c, d, e, f); false = no fit
__device__ bool fit_ellipse(const Poly& l, double* q) {
    if (l.n < 5) return false;
    double S1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, S2[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, S3[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < l.n; ++i) {
        const double x = l.x(i), y = l.y(i);
        const double d1[3] = {x * x, x * y, y * y}, d2[3] = {x, y, 1.0};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                S1[r * 3 + c] += d1[r] * d1[c];
                S2[r * 3 + c] += d1[r] * d2[c];
                S3[r * 3 + c] += d2[r] * d2[c];
            }
    }
    const double S2t[9] = {S2[0], S2[3], S2[6], S2[1], S2[4], S2[7], S2[2], S2[5], S2[8]};
    double T[9];
    if (!solve33(S3, S2t, T)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) T[i] = -T[i];
    double M[9];
    mul33(S2, T, M);
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = S1[i] + M[i];
    double A[9] = {M[6] / 2.0, M[7] / 2.0, M[8] / 2.0, -M[3], -M[4], -M[5], M[0] / 2.0, M[1] / 2.0, M[2] / 2.0};
    // eigenvalues of A: the characteristic cubic on the matrix scaled to unit size (the vectors do not change), each root then
    // polished by Newton steps on det(A - lam I) itself
    double sc = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) sc = fmax(sc, fabs(A[i]));
    if (!(sc > 0.0) || !(sc < INFINITY)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] /= sc;
    const double tr = A[0] + A[4] + A[8];
    const double c1 = (A[0] * A[4] - A[1] * A[3]) + (A[0] * A[8] - A[2] * A[6]) + (A[4] * A[8] - A[5] * A[7]);
    const double dt = det3(A);
    const double p = c1 - tr * tr / 3.0, g = -2.0 * tr * tr * tr / 27.0 + tr * c1 / 3.0 - dt;
    const double disc = g * g / 4.0 + p * p * p / 27.0;
    double lam[3];
    int nl;
    if (disc < 0.0) {
        const double m = 2.0 * sqrt(-p / 3.0);
        const double arg = fmin(1.0, fmax(-1.0, 3.0 * g / (p * m)));
        const double phi = acos(arg) / 3.0;
        const double third = 2.0943951023931953;          // 2 pi / 3
        lam[0] = m * cos(phi) + tr / 3.0;
        lam[1] = m * cos(phi - third) + tr / 3.0;
        lam[2] = m * cos(phi - 2.0 * third) + tr / 3.0;
        nl = 3;
    } else {
        const double sq = sqrt(disc);
        lam[0] = cbrt(-g / 2.0 + sq) + cbrt(-g / 2.0 - sq) + tr / 3.0;
        lam[1] = lam[2] = lam[0];
        nl = 1;
    }
    for (int e = 0; e < nl; ++e) {
        double lm = lam[e];
        for (int it = 0; it < 8; ++it) {
            const double B[9] = {A[0] - lm, A[1], A[2], A[3], A[4] - lm, A[5], A[6], A[7], A[8] - lm};
            const double f = det3(B);
            const double df = -((B[0] * B[4] - B[1] * B[3]) + (B[0] * B[8] - B[2] * B[6]) + (B[4] * B[8] - B[5] * B[7]));
            if (!(fabs(df) > 0.0)) break;
            const double step = f / df;
            if (!(fabs(step) < INFINITY)) break;
            lm -= step;
            if (fabs(step) <= 4e-16 * fmax(fabs(lm), 1e-300)) break;
        }
        // the null vector of A - lam I: the largest of the three cross products of its rows
        const double B[9] = {A[0] - lm, A[1], A[2], A[3], A[4] - lm, A[5], A[6], A[7], A[8] - lm};
        double best[3] = {0, 0, 0}, bn = -1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double* u = B + 3 * r;
            const double* w = B + 3 * ((r + 1) % 3);
            const double v[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
            if (n2 > bn) { bn = n2; best[0] = v[0]; best[1] = v[1]; best[2] = v[2]; }
        }
        if (!(bn > 0.0)) continue;
        const double nr = sqrt(bn);
        const double v[3] = {best[0] / nr, best[1] / nr, best[2] / nr};
        if (4.0 * v[0] * v[2] - v[1] * v[1] > 0.0) {
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
            mul3v(T, v, q + 3);
            return true;
        }
    }
    return false;
}

// conic_line_points: the conic on p0 + t d (homogeneous); 0 or 2 points, in the order of the two roots
__device__ int conic_line_points(const double* q, const double* p0, const double* d, double (&out)[2][2]) {
    const double C[9] = {q[0], q[1] / 2, q[3] / 2, q[1] / 2, q[2], q[4] / 2, q[3] / 2, q[4] / 2, q[5]};
    double dC[3], pC[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        dC[j] = d[0] * C[j] + d[1] * C[3 + j] + d[2] * C[6 + j];
        pC[j] = p0[0] * C[j] + p0[1] * C[3 + j] + p0[2] * C[6 + j];
    }
    const double qa = dC[0] * d[0] + dC[1] * d[1] + dC[2] * d[2];
    const double qb = 2.0 * (pC[0] * d[0] + pC[1] * d[1] + pC[2] * d[2]);
    const double qc = pC[0] * p0[0] + pC[1] * p0[1] + pC[2] * p0[2];
    if (fabs(qa) < 1e-300) return 0;
    const double disc = qb * qb - 4.0 * qa * qc;
    if (disc < 0.0) return 0;
    if (!(disc >= 0.0)) return 0;                          // NaN: numpy's sqrt would carry it on; such a conic gives no label either way
    const double s = sqrt(disc);
    const double t[2] = {(-qb - s) / (2 * qa), (-qb + s) / (2 * qa)};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double h0 = p0[0] + t[i] * d[0], h1 = p0[1] + t[i] * d[1], h2 = p0[2] + t[i] * d[2];
        out[i][0] = h0 / h2;
        out[i][1] = h1 / h2;
    }
    return 2;
}

// tangent_points; false = no real tangent
__device__ bool tangent_points(const double* q, double x0, double y0, double (&out)[2][2]) {
    const double a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
    const double l0 = a * x0 + b / 2 * y0 + d / 2, l1 = b / 2 * x0 + c * y0 + e / 2, l2 = d / 2 * x0 + e / 2 * y0 + f;
    double p0[3];
    const double dir[3] = {-l1, l0, 0.0};
    if (fabs(l0) >= fabs(l1)) { p0[0] = -l2 / l0; p0[1] = 0.0; p0[2] = 1.0; }
    else { p0[0] = 0.0; p0[1] = -l2 / l1; p0[2] = 1.0; }
    double pts[2][2];
    if (conic_line_points(q, p0, dir, pts) != 2) return false;
    const double s0 = (pts[0][1] - y0) / (pts[0][0] - x0), s1 = (pts[1][1] - y0) / (pts[1][0] - x0);
    const double csign = 4 * a * c * (x0 * x0) - (b * b) * (x0 * x0) - 2 * b * e * x0 + 4 * c * d * x0 + 4 * c * f - e * e;
    const bool first_is_smaller = csign > 0;
    const bool rev = (s0 < s1) != first_is_smaller;
#pragma unroll
    for (int i = 0; i < 2; ++i) { out[i][0] = pts[rev ? 1 - i : i][0]; out[i][1] = pts[rev ? 1 - i : i][1]; }
    return true;
}

__device__ int cut(const double* q, const Poly& poly, double (&out)[2][2]) {
    const double x0 = poly.x(0);
    if (is_vertical(poly, x0)) {
        const double p0[3] = {x0, 0.0, 1.0}, d[3] = {0.0, 1.0, 0.0};
        return conic_line_points(q, p0, d, out);
    }
    double k, h;
    fit_slope(poly, k, h);
    const double p0[3] = {0.0, h, 1.0}, d[3] = {1.0, k, 0.0};
    return conic_line_points(q, p0, d, out);
}

__device__ bool conic_cross_line(const double* q, const Poly& line, double (&out)[2][2]) {
    double first[2][2];
    if (cut(q, line, first) != 2) return false;
    const bool sw = first[1][0] < first[0][0] || (first[1][0] == first[0][0] && first[1][1] < first[0][1]);      // sorted by (x, y)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double px = first[sw ? 1 - i : i][0], py = first[sw ? 1 - i : i][1];
        Poly seg;
        if (two_nearest_bracket(line, px, py, seg) && fabs(seg.ax - seg.bx) > 0.0) {
            double k, h, cand[2][2];
            fit_slope(seg, k, h);
            const double p0[3] = {0.0, h, 1.0}, d[3] = {1.0, k, 0.0};
            if (conic_line_points(q, p0, d, cand) == 2) {
                const double e0 = (cand[0][0] - px) * (cand[0][0] - px) + (cand[0][1] - py) * (cand[0][1] - py);
                const double e1 = (cand[1][0] - px) * (cand[1][0] - px) + (cand[1][1] - py) * (cand[1][1] - py);
                const int w = e1 < e0 ? 1 : 0;
                px = cand[w][0]; py = cand[w][1];
            }
        }
        out[i][0] = px; out[i][1] = py;
    }
    return true;
}

// pick_side: ci = 0 central, 1 left, 2 right; top = the 'Top' keypoint is asked for
__device__ void pick_side(const Frame& f, const double (&pair)[2][2], int ci, int circle_cls, int line_cls, bool top, double& ox, double& oy) {
    const double y_min = fmin(pair[0][1], pair[1][1]);
    bool left_right = false;
    for (int c = 0; c < LB_NCLS && !left_right; ++c) {
        if (!((LB_LEFT >> c) & 1u) || c == line_cls || c == circle_cls || !cls_key(f, c)) continue;
        const Poly l = cls_poly(f, c);
        for (int i = 0; i < l.n; ++i)
            if (l.y(i) > y_min) { left_right = true; break; }
    }
    if (ci != 0) {
        const Poly l = cls_poly(f, circle_cls);
        for (int i = 0; i < l.n && !left_right; ++i)
            if (ci == 1 ? (y_min - l.y(i)) > 3 : (l.y(i) - y_min) > 3) left_right = true;
    }
    const double dx = fabs(pair[0][0] - pair[1][0]), dy = fabs(pair[0][1] - pair[1][1]);
    int b, t;                                              // indices of bottom and top
    if (dy < 1.0 || dx / dy > 10) {
        if (pair[0][0] < pair[1][0]) { b = 1; t = 0; } else { b = 0; t = 1; }
        if (!left_right) { const int s = b; b = t; t = s; }
    } else {
        if (pair[0][1] < pair[1][1]) { b = 1; t = 0; } else { b = 0; t = 1; }
    }
    const int w = top ? t : b;
    ox = pair[w][0]; oy = pair[w][1];
}

// ---- the frame's shared state ------------------------------------------------------------------------------------
struct Shared {
    double lab[NKP][2];
    double kw[MAX_KNOWN][2], ki[MAX_KNOWN][2];             // known points: pitch and image, both rounded to fp32
    double N[9][9], V[9][9];
    double Hb[9];
    double ys[2][40];
    unsigned char pres[NKP];                               // 0 = None, 1 = a label (possibly NaN)
    unsigned char masked[NKP];
    int n_known;
    int swap;
};

// smallest eigenvector of the symmetric 9x9 S.N by cyclic Jacobi: lanes 0..8 each turn one row / column, barriers between the phases
__device__ void jacobi9_smallest(Shared& S, int lane, double (&h)[9]) {
    if (lane < 9)
        for (int j = 0; j < 9; ++j) S.V[lane][j] = lane == j ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 9; ++i) {
            diag += S.N[i][i] * S.N[i][i];
            for (int j = i + 1; j < 9; ++j) off += S.N[i][j] * S.N[i][j];
        }
        if (!(off > 1e-36 * diag)) break;                  // uniform: every lane reads the same matrix
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = S.N[p][q];
                double cs = 1.0, sn = 0.0;
                if (apq != 0.0) {
                    const double th = (S.N[q][q] - S.N[p][p]) / (2.0 * apq);
                    const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    cs = 1.0 / sqrt(tt * tt + 1.0);
                    sn = tt * cs;
                }
                __syncthreads();
                if (lane < 9) {
                    const double a = S.N[lane][p], b = S.N[lane][q];
                    S.N[lane][p] = cs * a - sn * b; S.N[lane][q] = sn * a + cs * b;
                    const double va = S.V[lane][p], vb = S.V[lane][q];
                    S.V[lane][p] = cs * va - sn * vb; S.V[lane][q] = sn * va + cs * vb;
                }
                __syncthreads();
                if (lane < 9) {
                    const double a = S.N[p][lane], b = S.N[q][lane];
                    S.N[p][lane] = cs * a - sn * b; S.N[q][lane] = sn * a + cs * b;
                }
                __syncthreads();
            }
    }
    int best = 0;
    for (int i = 1; i < 9; ++i)
        if (S.N[i][i] < S.N[best][best]) best = i;
    for (int i = 0; i < 9; ++i) h[i] = S.V[i][best];
    __syncthreads();
}

// _dlt's similarity: centroid and sqrt(2) / mean distance, over the lanes of `inl`
__device__ void dlt_norm(u64 inl, int lane, double x, double y, double& mx, double& my, double& s) {
    const bool in = (inl >> lane) & 1;
    const double n = (double)popc64(inl);
    mx = wsum(in ? x : 0.0) / n;
    my = wsum(in ? y : 0.0) / n;
    const double md = wsum(in ? sqrt((x - mx) * (x - mx) + (y - my) * (y - my)) : 0.0) / n;
    s = sqrt(2.0) / fmax(md, 1e-12);
}

// A four-point sample with exactly three collinear PITCH points (common: many template points share a line) has one exact solution
// of the host's DLT system, the rank-one matrix d4 l^T -- l the line through the three, d4 the fourth point's image -- and that is
// what the host's SVD returns: every pitch point off the line lands on d4, a point on it is 0 / 0.  Restated here so that a frame
// whose only hypothesis is of this kind (n == 4) gets the host's labels; any other degenerate sample is skipped (include/sncal.h).
__device__ bool rank_one_homography(const double (&s)[4][2], const double (&d)[4][2], double* H) {
    double mx = 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmax(mx, fmax(fabs(s[i][0]), fabs(s[i][1])));
    const double tol = 1e-9 * mx * mx;
    int off = -1, found = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {                          // m = the point left out of the triple
        const int i = m == 0 ? 1 : 0, j = m <= 1 ? 2 : 1, k = m == 3 ? 2 : 3;
        const double cr = (s[j][0] - s[i][0]) * (s[k][1] - s[i][1]) - (s[j][1] - s[i][1]) * (s[k][0] - s[i][0]);
        if (fabs(cr) < tol) { ++found; off = m; }
    }
    if (found != 1) return false;
    const int i = off == 0 ? 1 : 0, k = off == 3 ? 2 : 3;  // the triple's first and last point
    const double l[3] = {s[i][1] - s[k][1], s[k][0] - s[i][0], s[i][0] * s[k][1] - s[k][0] * s[i][1]};
    if (!(fabs(l[0]) + fabs(l[1]) > 0.0)) return false;
    const double u = off == 0 ? d[0][0] : off == 1 ? d[1][0] : off == 2 ? d[2][0] : d[3][0];
    const double v = off == 0 ? d[0][1] : off == 1 ? d[1][1] : off == 2 ? d[2][1] : d[3][1];
#pragma unroll
    for (int c = 0; c < 3; ++c) { H[c] = u * l[c]; H[3 + c] = v * l[c]; H[6 + c] = l[c]; }
    return true;
}
// x H^T in homogeneous coordinates -> (u, v); a denominator that is rounding noise of a point ON the line of a rank-one H reads as 0 / 0
__device__ inline void project(const double* H, double x, double y, double& u, double& v) {
    const double t0 = H[6] * x, t1 = H[7] * y, w = t0 + t1 + H[8];
    const bool noise = fabs(w) <= 1e-12 * (fabs(t0) + fabs(t1) + fabs(H[8]));
    u = noise ? NAN : (H[0] * x + H[1] * y + H[2]) / w;
    v = noise ? NAN : (H[3] * x + H[4] * y + H[5]) / w;
}

// homography_ransac over S.kw -> S.ki; true: H (row-major, H[8] = 1) is uniform over the wave
__device__ bool ransac(Shared& S, int lane, const unsigned char* __restrict__ samples, double* H) {
    const int n = S.n_known;
    if (n < 4) return false;
    const int iters = n > 4 ? RANSAC_ITERS : 1;
    const unsigned char* tab = samples + (size_t)n * RANSAC_ITERS * 4;
    int my_cnt = -1, my_h = 1 << 30;
    u64 my_inl = 0;
    double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int hyp = lane; hyp < iters; hyp += 64) {
        int idx[4] = {0, 1, 2, 3};
        if (n > 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) idx[k] = min((int)tab[hyp * 4 + k], n - 1);
        }
        double s[4][2], d[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s[k][0] = S.kw[idx[k]][0]; s[k][1] = S.kw[idx[k]][1];
            d[k][0] = S.ki[idx[k]][0]; d[k][1] = S.ki[idx[k]][1];
        }
        double Hh[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!homography_4pt(s, d, Hh) && !rank_one_homography(s, d, Hh)) continue;           // any other degenerate sample is skipped
        int cnt = 0;
        u64 inl = 0;
        for (int j = 0; j < n; ++j) {
            double pu, pv;
            project(Hh, S.kw[j][0], S.kw[j][1], pu, pv);
            pu -= S.ki[j][0]; pv -= S.ki[j][1];
            if (sqrt(pu * pu + pv * pv) < 5.0) { ++cnt; inl |= 1ull << j; }
        }
        if (cnt > my_cnt) {                                // ascending hypotheses per lane: the first of the highest count stays
            my_cnt = cnt; my_h = hyp; my_inl = inl;
#pragma unroll
            for (int i = 0; i < 9; ++i) Hm[i] = Hh[i];
        }
    }
    int bc = my_cnt, bh = my_h;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int qc = __shfl_xor(bc, o, 64), qh = __shfl_xor(bh, o, 64);
        if (qc > bc || (qc == bc && qh < bh)) { bc = qc; bh = qh; }
    }
    if (bc < 0) return false;
    const int owner = bh & 63;
    double Hbest[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hbest[i] = bcast(Hm[i], owner);
    const u64 inl = (u64)__shfl((long long)my_inl, owner, 64);
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = Hbest[i];
    if (bc < 4) return true;
    // the final fit: unit-norm normalised DLT on the inliers, lane j = known point j
    const bool in = lane < n && ((inl >> lane) & 1);
    const double sx = lane < n ? S.kw[lane][0] : 0.0, sy = lane < n ? S.kw[lane][1] : 0.0;
    const double du = lane < n ? S.ki[lane][0] : 0.0, dv = lane < n ? S.ki[lane][1] : 0.0;
    double msx, msy, ss, mdx, mdy, sd;
    dlt_norm(inl, lane, sx, sy, msx, msy, ss);
    dlt_norm(inl, lane, du, dv, mdx, mdy, sd);
    const double x = ss * sx + -ss * msx, y = ss * sy + -ss * msy, u = sd * du + -sd * mdx, v = sd * dv + -sd * mdy;
    const double r1[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
    const double r2[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int b = a; b < 9; ++b) {
            const double t = wsum(in ? r1[a] * r1[b] + r2[a] * r2[b] : 0.0);
            if (lane == 0) { S.N[a][b] = t; S.N[b][a] = t; }
        }
    __syncthreads();
    double h[9];
    jacobi9_smallest(S, lane, h);
    // H = inv(Td) @ Hn @ Ts
    const double Ts[9] = {ss, 0, -ss * msx, 0, ss, -ss * msy, 0, 0, 1};
    const double Ti[9] = {1 / sd, 0, mdx, 0, 1 / sd, mdy, 0, 0, 1};
    double t1[9], Hf[9];
    mul33(h, Ts, t1);
    mul33(Ti, t1, Hf);
    if (fabs(Hf[8]) > 1e-300) {
        const double s8 = Hf[8];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) { Hf[i] /= s8; fin = fin && (fabs(Hf[i]) < INFINITY); }
        if (fin) {
#pragma unroll
            for (int i = 0; i < 9; ++i) H[i] = Hf[i];
        }
    }
    return true;
}

// get_intersections for one frame: S.lab / S.pres after the final inside(), S.masked
__device__ void labels_pass(Shared& S, const Frame& f, int lane, bool within, double margin, const unsigned char* __restrict__ samples) {
    if (lane < NKP) { S.pres[lane] = 0; S.masked[lane] = 0; S.lab[lane][0] = 0.0; S.lab[lane][1] = 0.0; }
    __syncthreads();
    if (lane < 30) {
        const Poly l1 = cls_poly(f, LB_LINE[lane][0]), l2 = cls_poly(f, LB_LINE[lane][1]);
        double x, y;
        if (l1.n > 1 && l2.n > 1 && line_intersection(l1, l2, x, y) && inside(x, y, f.W, f.H, within, margin)) {
            S.lab[lane][0] = x; S.lab[lane][1] = y; S.pres[lane] = 1;
        }
    }
    __syncthreads();
    if (lane < 3) {
        const int ccls = LB_CIRCLE[lane];
        const Poly circle = cls_poly(f, ccls);
        double q[6];
        if (circle.n > 4 && fit_ellipse(circle, q)) {
            for (int e = 0; e < LB_NCONIC; ++e) {
                if (LB_CONIC[e][0] != lane) continue;
                const int kid = LB_CONIC[e][1], arg = LB_CONIC[e][3], sel = LB_CONIC[e][4];
                if (LB_CONIC[e][2] == 0) {
                    if (S.pres[arg]) {
                        double tp[2][2];
                        if (tangent_points(q, S.lab[arg][0], S.lab[arg][1], tp)) { S.lab[kid][0] = tp[sel][0]; S.lab[kid][1] = tp[sel][1]; }
                        else { S.lab[kid][0] = NAN; S.lab[kid][1] = NAN; }
                        S.pres[kid] = 1;
                    }
                } else {
                    const Poly line = cls_poly(f, arg);
                    double pair[2][2];
                    if (line.n > 1 && conic_cross_line(q, line, pair)) {
                        double ox, oy;
                        pick_side(f, pair, lane, ccls, arg, sel == 1, ox, oy);
                        S.lab[kid][0] = ox; S.lab[kid][1] = oy; S.pres[kid] = 1;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        int n = 0;
        for (int e = 0; e < LB_NORDER; ++e) {
            const int i = LB_ORDER[e];
            if (!S.pres[i] || ((LB_NOT_ON_PLANE >> i) & 1ull) || !(S.lab[i][0] == S.lab[i][0])) continue;
            S.kw[n][0] = (double)(float)LB_PITCH[i][0]; S.kw[n][1] = (double)(float)LB_PITCH[i][1];
            S.ki[n][0] = (double)(float)S.lab[i][0]; S.ki[n][1] = (double)(float)S.lab[i][1];
            ++n;
        }
        S.n_known = n;
    }
    __syncthreads();
    double H[9];
    const bool have = ransac(S, lane, samples, H);
    __syncthreads();
    if (lane < 27) {
        const int i = 30 + lane;
        if (!S.pres[i]) {
            if (have) {
                project(H, LB_PITCH[i][0], LB_PITCH[i][1], S.lab[i][0], S.lab[i][1]);
                S.pres[i] = 1;
            } else {
                S.masked[i] = 1;
            }
        }
    }
    __syncthreads();
    if (lane < NKP && S.pres[lane] && !inside(S.lab[lane][0], S.lab[lane][1], f.W, f.H, true, margin)) S.pres[lane] = 0;
    __syncthreads();
}

// FixLRAmbiguous.decide on the labels of a margin-0 pass (one lane)
__device__ bool decide_swap(Shared& S, unsigned present) {
    const int n_left = __popc(present & LB_LEFT), n_right = __popc(present & LB_RIGHT);
    int n_total = 0, n_horizontal = 0, nl = 0, nr = 0;
    for (int e = 0; e < LB_NPERP; ++e) {
        const int a = LB_PERP[e][0], b = LB_PERP[e][1];
        if (!S.pres[a] || !S.pres[b]) continue;
        ++n_total;
        for (int k = 0; k < 2; ++k) {
            const int i = k == 0 ? a : b;
            if ((LB_POINTS_LEFT >> i) & 1ull) S.ys[0][nl++] = S.lab[i][1];
            else if ((LB_POINTS_RIGHT >> i) & 1ull) S.ys[1][nr++] = S.lab[i][1];
        }
        const double dx = fabs(S.lab[a][0] - S.lab[b][0]), dy = fabs(S.lab[a][1] - S.lab[b][1]);
        if (dy < 1.0 || dx / dy > 10.0) ++n_horizontal;
    }
    if (!(n_total > 0 && 2 * n_horizontal >= n_total)) return false;
    if (nl > 0 && nr > 0) {
        double med[2];
        for (int s = 0; s < 2; ++s) {
            const int n = s == 0 ? nl : nr;
            double* v = S.ys[s];
            for (int i = 1; i < n; ++i) {
                const double t = v[i];
                int j = i - 1;
                while (j >= 0 && v[j] > t) { v[j + 1] = v[j]; --j; }
                v[j + 1] = t;
            }
            med[s] = (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
        }
        return med[0] < med[1];
    }
    return n_right > n_left;
}

__global__ __launch_bounds__(64) void keypoint_labels_kernel(const double* __restrict__ pts, int total, const int* __restrict__ offsets,
                                                             const unsigned* __restrict__ present, int img_w, int img_h, int within,
                                                             double margin, int N, unsigned flags,
                                                             const unsigned char* __restrict__ samples, float* __restrict__ rows,
                                                             long long* __restrict__ mask, double* __restrict__ labels,
                                                             unsigned char* __restrict__ label_present, unsigned char* __restrict__ swapped) {
    __shared__ Shared S;
    const int b = blockIdx.x, lane = threadIdx.x;
    Frame f;
    f.pts = pts;
    f.off = offsets + (size_t)b * (LB_NCLS + 1);
    f.total = total;
    f.present = present[b];
    f.swap = false;
    f.W = (double)img_w; f.H = (double)img_h;
    const bool fix = flags & FLAG_FIX_LR;
    if (fix) {
        labels_pass(S, f, lane, true, 0.0, samples);       // decide()'s get_intersections: within_image, margin 0
        if (lane == 0) S.swap = decide_swap(S, f.present) ? 1 : 0;
        __syncthreads();
        f.swap = S.swap != 0;
        if (f.swap || margin != 0.0 || !within) labels_pass(S, f, lane, within != 0, margin, samples);
    } else {
        labels_pass(S, f, lane, within != 0, margin, samples);
    }
    if (lane == 0 && swapped) swapped[b] = f.swap ? 1 : 0;
    if (lane < N) {
        const bool p = S.pres[lane];
        float* r = rows + ((size_t)b * N + lane) * 3;
        r[0] = p ? (float)S.lab[lane][0] : -1.0f;
        r[1] = p ? (float)S.lab[lane][1] : -1.0f;
        r[2] = p ? 1.0f : 0.0f;
    }
    if (lane <= N) mask[(size_t)b * (N + 1) + lane] = (lane < NKP && S.masked[lane]) ? 0 : 1;
    if (labels && lane < NKP) {
        const bool p = S.pres[lane];
        labels[((size_t)b * NKP + lane) * 2] = p ? S.lab[lane][0] : NAN;
        labels[((size_t)b * NKP + lane) * 2 + 1] = p ? S.lab[lane][1] : NAN;
        label_present[(size_t)b * NKP + lane] = p ? 1 : 0;
    }
}

}  // namespace

extern "C" int sncal_keypoint_labels_workspace(int B, int total_points, size_t* bytes) {
    SNCAL_CHECK_ARG(bytes, "sncal_keypoint_labels_workspace: null pointer");
    SNCAL_CHECK_ARG(B >= 0 && total_points >= 0, "sncal_keypoint_labels_workspace: B=%d total_points=%d", B, total_points);
    *bytes = 0;                                            // a frame's state fits its workgroup's LDS; polylines are read in place
    return SNCAL_OK;
}

extern "C" int sncal_keypoint_labels(const double* d_points, int total_points, const int* d_offsets, const unsigned* d_present, int B,
                                     int n_classes, int img_w, int img_h, int within_image, double margin, int num_keypoints,
                                     unsigned flags, const unsigned char* d_samples, float* d_keypoints, long long* d_mask,
                                     double* d_labels, unsigned char* d_label_present, unsigned char* d_swapped, void* d_ws,
                                     size_t ws_bytes, void* stream) {
    (void)d_ws; (void)ws_bytes;
    SNCAL_CHECK_ARG(B >= 0 && total_points >= 0, "sncal_keypoint_labels: B=%d total_points=%d", B, total_points);
    SNCAL_CHECK_ARG(n_classes == LB_NCLS, "sncal_keypoint_labels: n_classes=%d, the class order has %d", n_classes, LB_NCLS);
    SNCAL_CHECK_ARG(num_keypoints >= 1 && num_keypoints <= NKP, "sncal_keypoint_labels: num_keypoints=%d (1..%d)", num_keypoints, NKP);
    SNCAL_CHECK_ARG(img_w >= 1 && img_h >= 1, "sncal_keypoint_labels: image %d x %d", img_w, img_h);
    SNCAL_CHECK_ARG(margin == margin, "sncal_keypoint_labels: margin is NaN");
    SNCAL_CHECK_ARG((flags & ~FLAG_FIX_LR) == 0, "sncal_keypoint_labels: unknown flags 0x%x", flags);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_offsets && d_present && d_samples && d_keypoints && d_mask, "sncal_keypoint_labels: null pointer");
    SNCAL_CHECK_ARG(d_points || total_points == 0, "sncal_keypoint_labels: null points");
    SNCAL_CHECK_ARG(!d_labels == !d_label_present, "sncal_keypoint_labels: d_labels and d_label_present come together");
    SNCAL_CHECK_ARG(!(flags & FLAG_FIX_LR) || d_swapped, "sncal_keypoint_labels: SNCAL_LABELS_FIX_LR needs d_swapped");
    hipLaunchKernelGGL(keypoint_labels_kernel, dim3(B), dim3(64), 0, sncal::as_stream(stream), d_points, total_points, d_offsets, d_present, img_w,
                       img_h, within_image, margin, num_keypoints, flags, d_samples, d_keypoints, d_mask, d_labels, d_label_present,
                       d_swapped);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
