// Cameras from line extremities on the device: the dev-kit's baseline of the calibration task, a batch in one launch.
//   baseline/baseline_cameras.py:13-41    normalization_transform            (sim_of: the running mean, in the reference's order)
//   baseline/baseline_cameras.py:44-106   estimate_homography_from_line_correspondences (stage 3: rows, SVD, vector choice)
//   baseline/baseline_cameras.py:174-246  __main__ per frame: candidates, line matches, Camera.from_homography, nearest candidates,
//                                         Camera.refine_camera
//   baseline/camera.py:121-154, 249-268   from_homography, project_point (float32 normalised coordinates, :247)
// baseline_cameras.py (the package's) restates the same flow on the host and is the specification; what differs here is the order
// of a few sums, the closed forms of the 3x3 inverses and the SVD, i.e. rounding.
//
// One workgroup of one wavefront per frame, registers only (no LDS, no workspace), fp64 without contraction.  line_cameras_kernel:
//   1. classes   lane c < 28 owns class c (ANNOT_CLASSES order): its first two points in pixels, kept / lawn-line flags by ballot
//   2. T1, T2    serial walks over the kept classes in class order, the same in every lane (wave-uniform)
//   3. SVD       lane r < 2L owns row r of the 2L x 9 system (L <= 17), lanes 48..56 the rows of V; one-sided (Hestenes) Jacobi: the
//                nine columns in registers, a column pair's three products by wave sums, the rotation applied to A and V alike
//   4. camera    from_homography in every lane; lane e < 34 owns 3-D end point e: projection, nearest candidate, the 100 px rule
// line_refine_kernel (refine = 1), behind it on the stream:
//   5. refine    the pose LM of sncal_pnp_refine_lm (solve_pose.hpp) on the matches, lane e holding match e
// Plain stores, no atomics: a frame's record depends on neither the batch size nor its position in it.
#include "common.hpp"
#include <cstdint>
#include <cmath>
#include <cstring>

typedef unsigned long long u64;
#include "solve_wave.hpp"
#include "solve_linalg.hpp"
#include "solve_homography.hpp"
#include "solve_pose.hpp"

namespace {

#include "linecam_tables.inc"

constexpr int LC_FIRST_LINE = 3, LC_MAX_PEAK_C = 23, LC_CENTRAL = 0;
constexpr int LC_VLANE = 48;                   // lanes 48..56 hold the rows of V
constexpr int LC_MAX_SWEEPS = 30;
constexpr double LC_MATCH_PX = 100.0;
static_assert(LC_NCLS <= 32 && LC_NPTS <= LC_VLANE && 2 * LC_NCLS <= 64, "lane layout");

struct Sim { double s, tx, ty; };              // [[s, 0, tx], [0, s, ty], [0, 0, 1]]

__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// normalization_transform (:13-41) of a cloud given as a walk: `walk(f)` calls f(x, y) for every point, in order
template <class Walk>
__device__ __forceinline__ Sim sim_of(Walk walk) {
    double sx = 0.0, sy = 0.0;
    int n = 0;
    walk([&](double x, double y) { sx += x; sy += y; ++n; });
    const double cx = sx / (double)n, cy = sy / (double)n;
    double d = 0.0;
    int k = 0;
    walk([&](double x, double y) {
        ++k;
        const double dx = x - cx, dy = y - cy;
        d += (sqrt(dx * dx + dy * dy) - d) / (double)k;
    });
    const double s = d <= 0.0 ? 1.0 : sqrt(2.0) / d;
    return Sim{s, -s * cx, -s * cy};
}

// inv(T)^T l for a similarity T (:56-57)
__device__ __forceinline__ void map_line(const Sim& T, const double* l, double* o) {
    const double i00 = 1.0 / T.s, i02 = -T.tx / T.s, i12 = -T.ty / T.s;
    o[0] = i00 * l[0];
    o[1] = i00 * l[1];
    o[2] = i02 * l[0] + i12 * l[1] + l[2];
}

// np.cross([ax, ay, 1], [bx, by, 1])
__device__ __forceinline__ void join(double ax, double ay, double bx, double by, double* l) {
    l[0] = ay * 1.0 - 1.0 * by;
    l[1] = 1.0 * bx - ax * 1.0;
    l[2] = ax * by - ay * bx;
}

// One-sided Jacobi on the wave: lane's row a[9] of [A; V]; `rowlane` marks the rows of A.  On return the columns of A are
// orthogonal, nrm[j] their norms (the singular values, unsorted) and the V lanes hold the right singular vectors as columns.
__device__ __forceinline__ void hestenes9(double (&a)[9], bool rowlane, double (&nrm)[9]) {
    for (int sweep = 0; sweep < LC_MAX_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double alpha = wsum_w<64>(rowlane ? a[p] * a[p] : 0.0);
                const double beta = wsum_w<64>(rowlane ? a[q] * a[q] : 0.0);
                const double gamma = wsum_w<64>(rowlane ? a[p] * a[q] : 0.0);
                if (gamma != 0.0 && fabs(gamma) > DBL_EPS * sqrt(alpha * beta)) {          // (wave-uniform; false for a NaN)
                    rotated = true;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                    const double ap = a[p], aq = a[q];
                    a[p] = c * ap - s * aq;
                    a[q] = s * ap + c * aq;
                }
            }
        }
        if (!rotated) break;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) nrm[j] = sqrt(wsum_w<64>(rowlane ? a[j] * a[j] : 0.0));
}

// the prediction of a call, in one of its two forms
struct Input {
    const float* peaks; int C; float scale, p_threshold;
    const double* pts; int total; const int* off;
};
struct ClassPoints { bool kept; double p[4]; };        // p1x, p1y, p2x, p2y in pixels

// the first two points of class c of frame b in pixels (:186-189), or kept = false: a class without extremities, 'Circle central',
// a class with fewer than two points
__device__ __forceinline__ ClassPoints class_points(const Input& in, int b, int c, double W, double Hh) {
    ClassPoints o = {false, {0.0, 0.0, 0.0, 0.0}};
    if (!(c >= 0 && c < LC_NCLS && c != LC_CENTRAL && LC_END[c][0] >= 0)) return o;
    if (in.peaks) {
        const int k = c - LC_FIRST_LINE;
        if (k >= 0 && k < in.C) {
            const float* r = in.peaks + ((size_t)b * in.C + k) * 6;
            if (r[2] >= in.p_threshold && r[5] >= in.p_threshold) {                        // both slots: a class needs two points
                o.kept = true;
                // the extremities_<id>.json value of the fp32 pixel (divided by W - 1, H - 1), read as the baseline reads it
                o.p[0] = (double)(r[0] * in.scale) / (W - 1.0) * W; o.p[1] = (double)(r[1] * in.scale) / (Hh - 1.0) * Hh;
                o.p[2] = (double)(r[3] * in.scale) / (W - 1.0) * W; o.p[3] = (double)(r[4] * in.scale) / (Hh - 1.0) * Hh;
            }
        }
    } else {
        const int* o_ = in.off + (size_t)b * (LC_NCLS + 1);
        const int lo = o_[c], hi = o_[c + 1];
        if (lo >= 0 && hi <= in.total && hi - lo >= 2) {                                   // fewer than two points: skipped
            o.kept = true;
            const double* q = in.pts + 2 * (size_t)lo;
            o.p[0] = q[0] * W; o.p[1] = q[1] * Hh; o.p[2] = q[2] * W; o.p[3] = q[3] * Hh;
        }
    }
    return o;
}

__global__ __launch_bounds__(64) void line_cameras_kernel(Input in, int B, int img_w, int img_h, sncal_camera* __restrict__ d_cam,
                                                          int32_t* __restrict__ d_status, double* __restrict__ d_H,
                                                          int32_t* __restrict__ d_nlines, int32_t* __restrict__ d_slots) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const double W = (double)img_w, Hh = (double)img_h;

    // ---- 1. the lane's class: its first two points in pixels (:183-206) ----
    const ClassPoints cp = class_points(in, b, lane, W, Hh);
    const bool kept = cp.kept;
    const double p1x = cp.p[0], p1y = cp.p[1], p2x = cp.p[2], p2y = cp.p[3];
    double img_line[3];
    join(p1x, p1y, p2x, p2y, img_line);
    const bool has_line = kept && ((LC_LAWN >> lane) & 1u) && isfinite((img_line[0] + img_line[1]) + img_line[2]);
    const unsigned kept_mask = (unsigned)__ballot(kept), line_mask = (unsigned)__ballot(has_line);
    const int L = __popc(line_mask);

    int status = SNCAL_LINECAM_NONE, n_match = 0, slot = -1;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, pos[3] = {0, 0, 0}, f = 0.0, rmse = 0.0;
    const double cx = W / 2.0, cy = Hh / 2.0;
    bool have_h = false;

    if (L >= 4) {
        // ---- 2. the two normalisations (:212-214): the distinct 3-D end points in their order of first appearance, the image cloud ----
        const Sim T1 = sim_of([&](auto f_) {
            u64 seen = 0;
            for (unsigned m = kept_mask; m; m &= m - 1) {
                const int c = __ffs(m) - 1;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int id = LC_END[c][e];
                    if (!((seen >> id) & 1)) { seen |= 1ull << id; f_(LC_POINT[id][0], LC_POINT[id][1]); }
                }
            }
        });
        const Sim T2 = sim_of([&](auto f_) {
            for (unsigned m = kept_mask; m; m &= m - 1) {
                const int c = __ffs(m) - 1;
                f_(bcast(p1x, c), bcast(p1y, c));
                f_(bcast(p2x, c), bcast(p2y, c));
            }
        });
        if (finite3(T1.s, T1.tx, T1.ty) && finite3(T2.s, T2.tx, T2.ty)) {
            // ---- 3. the 2L x 9 system (:53-84), its SVD and the vector of :87-97 ----
            const bool rowlane = lane < 2 * L;
            double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            {
                int c = 0;
                unsigned m = line_mask;
                for (int i = 0; i < (rowlane ? lane >> 1 : 0); ++i) m &= m - 1;           // (per-lane trip count, once per frame)
                c = rowlane ? __ffs(m) - 1 : 0;
                double tl[3] = {__shfl(img_line[0], c, 64), __shfl(img_line[1], c, 64), __shfl(img_line[2], c, 64)};
                if (rowlane) {
                    const int e0 = LC_END[c][0], e1 = LC_END[c][1];
                    double pl[3], s_[3], t_[3];
                    join(LC_POINT[e0][0], LC_POINT[e0][1], LC_POINT[e1][0], LC_POINT[e1][1], pl);
                    map_line(T1, pl, s_);
                    map_line(T2, tl, t_);
                    const double u = s_[0], v = s_[1], w = s_[2], x = t_[0], y = t_[1], z = t_[2];
                    if (lane & 1) { a[0] = x * w; a[2] = -x * u; a[3] = y * w; a[5] = -u * y; a[6] = z * w; a[8] = -u * z; }
                    else          { a[1] = x * w; a[2] = -x * v; a[4] = y * w; a[5] = -v * y; a[7] = z * w; a[8] = -v * z; }
                }
            }
            if (lane >= LC_VLANE && lane < LC_VLANE + 9) a[lane - LC_VLANE] = 1.0;
            double nrm[9];
            hestenes9(a, rowlane, nrm);
            // index min(2L, 9) - 1 of the values sorted descending, walking up past exact zeros; equal values keep column order
            int chosen = -1;
            for (int want = min(2 * L, 9) - 1; want >= 0 && chosen < 0; --want) {
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    int rank = 0;
#pragma unroll
                    for (int k = 0; k < 9; ++k) rank += (nrm[k] > nrm[j] || (nrm[k] == nrm[j] && k < j)) ? 1 : 0;
                    if (rank == want && nrm[j] > 0.0) chosen = j;
                }
            }
            if (chosen >= 0) {
                double mine = 0.0;
#pragma unroll
                for (int j = 0; j < 9; ++j) mine = chosen == j ? a[j] : mine;
                double V[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) V[j] = __shfl(mine, LC_VLANE + j, 64);
                const double T2i[9] = {1.0 / T2.s, 0, -T2.tx / T2.s, 0, 1.0 / T2.s, -T2.ty / T2.s, 0, 0, 1};
                const double T1m[9] = {T1.s, 0, T1.tx, 0, T1.s, T1.ty, 0, 0, 1};
                double M[9];
                mul33(T2i, V, M);
                mul33(M, T1m, H);
                const double h22 = H[8];
                bool fin = true;
#pragma unroll
                for (int i = 0; i < 9; ++i) { H[i] /= h22; fin = fin && isfinite(H[i]); }
                have_h = fin;
            }
        }
    }

    double X[3] = {0, 0, 0}, mu = 0.0, mv = 0.0;
    bool matched = false;
    if (have_h) {
        // ---- 4. Camera.from_homography (camera.py:121-154): no sign test on the translation, as there ----
        double fx, fy;
        bool ok = k_from_homography(H, cx, cy, fx, fy);
        if (ok) {
            const double Ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
            double hp[9];
            mul33(Ki, H, hp);
            const double l1 = 1.0 / sqrt(hp[0] * hp[0] + hp[3] * hp[3] + hp[6] * hp[6]);
            const double l2 = 1.0 / sqrt(hp[1] * hp[1] + hp[4] * hp[4] + hp[7] * hp[7]);
            const double l3 = sqrt(l1 * l2);
            const double r0[3] = {hp[0] * l1, hp[3] * l1, hp[6] * l1}, r1[3] = {hp[1] * l2, hp[4] * l2, hp[7] * l2};
            const double r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
            R[0] = r0[0]; R[1] = r1[0]; R[2] = r2[0];
            R[3] = r0[1]; R[4] = r1[1]; R[5] = r2[1];
            R[6] = r0[2]; R[7] = r1[2]; R[8] = r2[2];
            polar3(R);                                                                     // the nearest rotation (u @ vh of :146-150)
            const double t[3] = {hp[2] * l3, hp[5] * l3, hp[8] * l3};
            pos[0] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
            pos[1] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
            pos[2] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
#pragma unroll
            for (int i = 0; i < 9; ++i) ok = ok && isfinite(R[i]);
            ok = ok && finite3(pos[0], pos[1], pos[2]) && isfinite(fx);
        }
        if (ok) {
            status = SNCAL_LINECAM_HOMOGRAPHY;
            f = fx;
            // ---- the nearest candidate of every 3-D end point that projects inside the image (:222-236) ----
            const bool mine = lane < LC_NPTS;
            const int e = mine ? lane : 0;
            X[0] = LC_POINT[e][0]; X[1] = LC_POINT[e][1]; X[2] = LC_POINT[e][2];
            const double d[3] = {X[0] - pos[0], X[1] - pos[1], X[2] - pos[2]};
            double rc[3];
            mul3v(R, d, rc);
            bool inside = false;
            double qx = 0.0, qy = 0.0;
            if (mine && !(rc[2] <= 1e-3)) {
                qx = (double)(float)(rc[0] / rc[2]) * f + cx;                               // distort() returns float32 (camera.py:247)
                qy = (double)(float)(rc[1] / rc[2]) * f + cy;
                inside = 0.0 < qx && qx < W && 0.0 < qy && qy < Hh;
            }
            double dmin = 0.0;
            bool any = false, stop = false;                                               // np.argmin: the first minimum, or the first NaN
            for (unsigned m = kept_mask; m; m &= m - 1) {
                const int c = __ffs(m) - 1;
                const double ax = bcast(p1x, c), ay = bcast(p1y, c), bx = bcast(p2x, c), by = bcast(p2y, c);
                const bool cand = inside && (LC_END[c][0] == e || LC_END[c][1] == e);
#pragma unroll
                for (int end = 0; end < 2; ++end) {
                    const double px = end ? bx : ax, py = end ? by : ay;
                    const double dist = sqrt((qx - px) * (qx - px) + (qy - py) * (qy - py));
                    if (cand && !stop && (!any || dist < dmin || isnan(dist))) {
                        any = true; dmin = dist; slot = c * 2 + end; mu = px; mv = py;
                        stop = isnan(dist);
                    }
                }
            }
            matched = any && dmin < LC_MATCH_PX;
            if (!matched) slot = -1;
            const u64 mm = __ballot(matched);
            n_match = popc64(mm);
            const K4 k{f, f, cx, cy};
            double t[3];
            mul3v(R, pos, t);
            t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2];
            if (n_match > 0) {
                double z;
                const double e2 = reproj_e2(R, t, k, X, mu, mv, &z);
                rmse = wsum(matched ? sqrt(e2) : 0.0) / (double)n_match;
            }
        }
    }

    // ---- the record ----
    if (lane < LC_NPTS) d_slots[(size_t)b * LC_NPTS + lane] = status != SNCAL_LINECAM_NONE ? slot : -1;
    if (lane == 0) {
        sncal_camera o;
        memset(&o, 0, sizeof(o));
        if (status != SNCAL_LINECAM_NONE) {
            for (int i = 0; i < 3; ++i) o.position[i] = pos[i];
            for (int i = 0; i < 9; ++i) o.rotation[i] = R[i];
            o.fx = f; o.fy = f; o.cx = cx; o.cy = cy; o.rmse = rmse;
            o.status = status; o.n_points = n_match;
        }
        d_cam[b] = o;
        d_status[b] = status;
        d_nlines[b] = L;
        for (int i = 0; i < 9; ++i) d_H[(size_t)b * 9 + i] = have_h ? H[i] : 0.0;
    }
}

// ---- 5. Camera.refine_camera (camera.py:105-119) with more than 3 matches (:238-239) ----
// A kernel of its own, after line_cameras_kernel on the same stream: a frame's matches are rebuilt from its record (the slots, the
// camera) and the input, lane e holding the match of 3-D end point e.  (Inside the first kernel the per-lane state of a frame would
// have to stay live across the minimiser's out-of-line call; at that kernel's 512 registers the register allocator parked such
// values in accumulator registers from inside the divergent loop of lm_solver_pose_packed, i.e. for some lanes only.)
__global__ __launch_bounds__(64) void line_refine_kernel(Input in, int B, int img_w, int img_h, int sched, sncal_camera* __restrict__ d_cam,
                                                         int32_t* __restrict__ d_status, const int32_t* __restrict__ d_slots) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const double W = (double)img_w, Hh = (double)img_h;
    if (d_status[b] != SNCAL_LINECAM_HOMOGRAPHY || d_cam[b].n_points <= 3) return;            // (wave-uniform)
    const sncal_camera rec = d_cam[b];
    const int slot = lane < LC_NPTS ? d_slots[(size_t)b * LC_NPTS + lane] : -1;
    const bool matched = slot >= 0;
    const int e = lane < LC_NPTS ? lane : 0;
    const double X[3] = {LC_POINT[e][0], LC_POINT[e][1], LC_POINT[e][2]};
    const ClassPoints cp = class_points(in, b, matched ? slot >> 1 : -1, W, Hh);
    const double mu = cp.p[(slot & 1) * 2], mv = cp.p[(slot & 1) * 2 + 1];
    const u64 mm = __ballot(matched);
    const int n_match = popc64(mm);
    double R[9], pos[3], t[3];
    for (int i = 0; i < 9; ++i) R[i] = rec.rotation[i];
    for (int i = 0; i < 3; ++i) pos[i] = rec.position[i];
    mul3v(R, pos, t);
    t[0] = -t[0]; t[1] = -t[1]; t[2] = -t[2];
    const K4 k{rec.fx, rec.fy, rec.cx, rec.cy};
    if (sched == SCHED_OPENCV) lm_solver_pose_auto(mm, R, t, k, X, mu, mv, 20000, 1e-5);      // sncal_pnp_refine_lm's defaults
    else refine_pose_lm(mm, R, t, k, X, mu, mv, 100, 1e-10);
    double z;
    const double e2 = reproj_e2(R, t, k, X, mu, mv, &z);
    const double rmse = wsum(matched ? sqrt(e2) : 0.0) / (double)n_match;
    if (lane == 0) {
        sncal_camera o = rec;
        for (int i = 0; i < 9; ++i) o.rotation[i] = R[i];
        o.position[0] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
        o.position[1] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
        o.position[2] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
        o.rmse = rmse;
        o.status = SNCAL_LINECAM_REFINED;
        d_cam[b] = o;
        d_status[b] = SNCAL_LINECAM_REFINED;
    }
}

int env_schedule() {      // SNCAL_SOLVE_SCHEDULE, as sncal_pnp_refine_lm reads it
    const char* v = sncal::env_str(sncal::ENV_SOLVE_SCHEDULE);
    return v && !strcmp(v, "converged") ? SCHED_CONVERGED : SCHED_OPENCV;
}

}  // namespace

extern "C" int sncal_baseline_cameras(const float* d_peaks, int C, float scale, float p_threshold, const double* d_pred_points, int pred_total,
                                  const int* d_pred_offsets, int B, int n_classes, int img_w, int img_h, int refine,
                                  sncal_camera* d_cameras, int32_t* d_status, double* d_H, int32_t* d_n_lines, int32_t* d_slots,
                                  int n_slots, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && pred_total >= 0, "sncal_baseline_cameras: B=%d pred_total=%d", B, pred_total);
    SNCAL_CHECK_ARG(n_classes == LC_NCLS, "sncal_baseline_cameras: n_classes=%d, the class order has %d", n_classes, LC_NCLS);
    SNCAL_CHECK_ARG(n_slots == LC_NPTS, "sncal_baseline_cameras: n_slots=%d, the lines have %d distinct end points", n_slots, LC_NPTS);
    SNCAL_CHECK_ARG(img_w >= 2 && img_h >= 2, "sncal_baseline_cameras: image %d x %d", img_w, img_h);
    SNCAL_CHECK_ARG(refine == 0 || refine == 1, "sncal_baseline_cameras: refine=%d (0 or 1)", refine);
    SNCAL_CHECK_ARG(!d_peaks || (C >= 1 && C <= LC_MAX_PEAK_C), "sncal_baseline_cameras: C=%d (1..%d line channels)", C, LC_MAX_PEAK_C);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(!d_peaks != !(d_pred_points || d_pred_offsets),
                    "sncal_baseline_cameras: exactly one of d_peaks and d_pred_points / d_pred_offsets must be given");
    SNCAL_CHECK_ARG(d_cameras && d_status && d_H && d_n_lines && d_slots, "sncal_baseline_cameras: null output pointer");
    SNCAL_CHECK_ARG(d_peaks || (d_pred_offsets && (d_pred_points || pred_total == 0)), "sncal_baseline_cameras: null prediction points / offsets");
    const Input in{d_peaks, C, scale, p_threshold, d_pred_points, pred_total, d_pred_offsets};
    hipLaunchKernelGGL(line_cameras_kernel, dim3(B), dim3(64), 0, sncal::as_stream(stream), in, B, img_w, img_h, d_cameras, d_status, d_H,
                       d_n_lines, d_slots);
    SNCAL_CHECK_LAUNCH();
    if (!refine) return SNCAL_OK;
    hipLaunchKernelGGL(line_refine_kernel, dim3(B), dim3(64), 0, sncal::as_stream(stream), in, B, img_w, img_h, env_schedule(), d_cameras,
                       d_status, (const int32_t*)d_slots);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}
