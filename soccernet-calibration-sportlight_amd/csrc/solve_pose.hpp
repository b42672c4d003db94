// Part of the camera solve: included by solve.hip and by linecam.hip (one translation unit each), after solve_homography.hpp.
// Camera pose from point matches, K fixed: the pose of a plane homography, residual and Jacobian rows, the four minimisers
// (refine_pose_lm, lm_solver_pose, cvlevmarq_pose, polish4) and the RANSAC PnP built from them.
#pragma once

namespace {

// ---- pose ----------------------------------------------------------------------------------------
__device__ bool pose_from_homography(const double* H, double fx, double fy, double cx, double cy, double* R, double* t) {
    const double Ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
    double hp[9];
    mul33(Ki, H, hp);
    const double n0 = sqrt(hp[0] * hp[0] + hp[3] * hp[3] + hp[6] * hp[6]);
    const double n1 = sqrt(hp[1] * hp[1] + hp[4] * hp[4] + hp[7] * hp[7]);
    if (n0 < 1e-300 || n1 < 1e-300) return false;
    const double l1 = 1 / n0, l2 = 1 / n1, l3 = sqrt(l1 * l2);
    double r0[3] = {hp[0] * l1, hp[3] * l1, hp[6] * l1}, r1[3] = {hp[1] * l2, hp[4] * l2, hp[7] * l2};
    t[0] = hp[2] * l3; t[1] = hp[5] * l3; t[2] = hp[8] * l3;
    if (t[2] < 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { r0[i] = -r0[i]; r1[i] = -r1[i]; t[i] = -t[i]; }
    }
    const double r2[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
    R[0] = r0[0]; R[1] = r1[0]; R[2] = r2[0];
    R[3] = r0[1]; R[4] = r1[1]; R[5] = r2[1];
    R[6] = r0[2]; R[7] = r1[2]; R[8] = r2[2];
    polar3(R);
    return true;
}

struct K4 { double fx, fy, cx, cy; };

__device__ __forceinline__ void cam_point(const double* R, const double* t, const double* X, double* Xc) {
    Xc[0] = X[0] * R[0] + X[1] * R[1] + X[2] * R[2] + t[0];
    Xc[1] = X[0] * R[3] + X[1] * R[4] + X[2] * R[5] + t[1];
    Xc[2] = X[0] * R[6] + X[1] * R[7] + X[2] * R[8] + t[2];
}
__device__ __forceinline__ double reproj_e2(const double* R, const double* t, const K4& k, const double* X, double u,
                                            double v, double* zout) {
    double Xc[3];
    cam_point(R, t, X, Xc);
    *zout = Xc[2];
    const double zs = fabs(Xc[2]) < 1e-12 ? 1e-12 : Xc[2];
    const double pu = k.fx * Xc[0] / zs + k.cx - u, pv = k.fy * Xc[1] / zs + k.cy - v;
    return pu * pu + pv * pv;
}

// pose rows: residual + Jacobian wrt (w, t) for the left perturbation R <- exp(w) R
__device__ __forceinline__ void pose_rows(const double* R, const double* t, double f_x, double f_y, double cx, double cy,
                                          const double* X, double u, double v, double (&ju)[6], double (&jv)[6],
                                          double& ru, double& rv, double& xn, double& yn) {
    double Xc[3];
    cam_point(R, t, X, Xc);
    const double z = fabs(Xc[2]) < 1e-12 ? 1e-12 : Xc[2];
    const double iz = 1.0 / z;                        // ONE division per point and evaluation (round 5: six, a fifth of an LM iteration's instructions)
    const double x = Xc[0] * iz, y = Xc[1] * iz;
    xn = x; yn = y;
    ru = f_x * x + cx - u; rv = f_y * y + cy - v;
    const double fxz = f_x * iz, fyz = f_y * iz;
    const double du[3] = {fxz, 0.0, -fxz * x}, dv[3] = {0.0, fyz, -fyz * y};
    ju[0] = du[2] * Xc[1] - du[1] * Xc[2]; ju[1] = du[0] * Xc[2] - du[2] * Xc[0]; ju[2] = du[1] * Xc[0] - du[0] * Xc[1];
    ju[3] = du[0]; ju[4] = du[1]; ju[5] = du[2];
    jv[0] = dv[2] * Xc[1] - dv[1] * Xc[2]; jv[1] = dv[0] * Xc[2] - dv[2] * Xc[0]; jv[2] = dv[1] * Xc[0] - dv[0] * Xc[1];
    jv[3] = dv[0]; jv[4] = dv[1]; jv[5] = dv[2];
}

__device__ __forceinline__ void apply_step(const double* R, const double* t, const double* step, double* Rn, double* tn) {
    double E[9];
    exp_so3(step, E);
    mul33(E, R, Rn);
    mul3v(E, t, tn);
    tn[0] += step[3]; tn[1] += step[4]; tn[2] += step[5];
}

// Camera.refine_camera (camera.py:105-119): LM over the pose, K fixed, to convergence
__device__ void refine_pose_lm(u64 mask, double* R, double* t, const K4& k, const double* X, double u, double v,
                               int max_iters, double eps) {
    const int lane = threadIdx.x & 63;
    const bool in = (mask >> lane) & 1;
    auto cost = [&](const double* R_, const double* t_) {
        double z;
        const double e2 = reproj_e2(R_, t_, k, X, u, v, &z);
        return wsum(in ? e2 : 0.0);
    };
    double lam = 1e-3;
    double c0 = cost(R, t);
    for (int it = 0; it < max_iters; ++it) {
        double ju[6], jv[6], ru, rv, xn, yn;
        pose_rows(R, t, k.fx, k.fy, k.cx, k.cy, X, u, v, ju, jv, ru, rv, xn, yn);
        double A[6][6], g[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) {
                const double s = wsum(in ? ju[i] * ju[j] + jv[i] * jv[j] : 0.0);
                A[i][j] = s; A[j][i] = s;
            }
            g[i] = -wsum(in ? ju[i] * ru + jv[i] * rv : 0.0);
        }
        bool improved = false;
        double step[6], dc = 0;
        for (int tr = 0; tr < 12; ++tr) {
            double Ad[6][6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) Ad[i][j] = A[i][j] + (i == j ? A[i][i] * lam : 0.0);
            if (!chol_solve<6>(Ad, g, step)) { lam *= 10; continue; }
            double Rn[9], tn[3];
            apply_step(R, t, step, Rn, tn);
            const double c1 = cost(Rn, tn);
            if (c1 < c0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = Rn[i];
                t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
                lam = fmax(lam * 0.1, 1e-15);
                dc = c0 - c1; c0 = c1; improved = true;
                break;
            }
            lam *= 10;
        }
        double smax = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) smax = fmax(smax, fabs(step[i]));
        if (!improved || smax < eps || dc <= 1e-16 * fmax(c0, 1e-30)) break;
    }
    polar3(R);
}

// ---- OpenCV's own minimiser schedules (opencv-python 4.7.0.72, restated from the upstream sources from memory: UNPINNED; shared
// specification with oracle/solve.py lm_solver_pose / cvlevmarq_pose / _joint_cvlevmarq).  Parameters are [rvec, tvec] (Rodrigues), as
// cv.projectPoints differentiates them; SCHED_OPENCV is the default since round 3, SCHED_CONVERGED the build's earlier specification.
constexpr int SCHED_OPENCV = 0, SCHED_CONVERGED = 1;

// residual + Jacobian wrt (rvec, tvec): R = exp(rvec), Jl = left_jacobian_so3(rvec) computed by the caller
__device__ __forceinline__ void pose_rows_rvec(const double* R, const double* Jl, const double* t, double f_x, double f_y, double cx,
                                               double cy, const double* X, double u, double v, double (&ju)[6], double (&jv)[6],
                                               double& ru, double& rv, double& xn, double& yn) {
    double Xr[3];
    const double zero[3] = {0, 0, 0};
    cam_point(R, zero, X, Xr);
    const double Xc[3] = {Xr[0] + t[0], Xr[1] + t[1], Xr[2] + t[2]};
    const double z = fabs(Xc[2]) < 1e-12 ? 1e-12 : Xc[2];
    const double x = Xc[0] / z, y = Xc[1] / z;
    xn = x; yn = y;
    ru = f_x * x + cx - u; rv = f_y * y + cy - v;
    const double du[3] = {f_x / z, 0.0, -f_x * x / z}, dv[3] = {0.0, f_y / z, -f_y * y / z};
    // d . (w x Xr) = w . (Xr x d): a rotation about the camera origin moves the ROTATED point only (tvec is its own parameter)
    const double wu[3] = {Xr[1] * du[2] - Xr[2] * du[1], Xr[2] * du[0] - Xr[0] * du[2], Xr[0] * du[1] - Xr[1] * du[0]};
    const double wv[3] = {Xr[1] * dv[2] - Xr[2] * dv[1], Xr[2] * dv[0] - Xr[0] * dv[2], Xr[0] * dv[1] - Xr[1] * dv[0]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ju[j] = wu[0] * Jl[j] + wu[1] * Jl[3 + j] + wu[2] * Jl[6 + j];
        jv[j] = wv[0] * Jl[j] + wv[1] * Jl[3 + j] + wv[2] * Jl[6 + j];
        ju[3 + j] = du[j]; jv[3 + j] = dv[j];
    }
}

// normal equations of the pose problem at x = [rvec, tvec]: A = J^T J, g = J^T r, S = |r|^2, rinf = |r|_inf (all wave-uniform)
// `rc` (optional): the rotation of x -- angle, sine, cosine, matrix.  A call with want_j = false FILLS it; a call with want_j = true and
// rc->valid USES it instead of recomputing: lm_solver_pose linearises an accepted step at exactly the point it has just evaluated, and
// the sine / cosine / matrix of the rotation vector were 40 % of that evaluation's clocks (SNCAL_LM_TIMING: 5.3k clk per Jacobian
// evaluation, 2.2k per trial on the 8-point fit).
struct RotCache { RotAngle q; double R[9]; bool valid; };
template <int W = 64>
__device__ void pose_normal_eq(u64 mask, const double* x, const K4& k, const double* X, double u, double v, bool want_j,
                               double (&A)[6][6], double (&g)[6], double& S, double& rinf, RotCache* rc = nullptr) {
    const int lane = threadIdx.x & 63;
    const bool in = (mask >> lane) & 1;
    double R[9], Jl[9];
    RotAngle q;
    if (rc != nullptr && want_j && rc->valid) {
        q = rc->q;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = rc->R[i];
    } else {
        q = rot_angle(x);
        exp_so3_a(x, q, R);
        if (rc != nullptr) {
            rc->q = q; rc->valid = true;
#pragma unroll
            for (int i = 0; i < 9; ++i) rc->R[i] = R[i];
        }
    }
    double ju[6], jv[6], ru, rv, xn, yn;
    if (want_j) {
        left_jacobian_so3_a(x, q, Jl);
        pose_rows_rvec(R, Jl, x + 3, k.fx, k.fy, k.cx, k.cy, X, u, v, ju, jv, ru, rv, xn, yn);
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
            for (int j = i; j < 6; ++j) {
                const double s = wsum_w<W>(in ? ju[i] * ju[j] + jv[i] * jv[j] : 0.0);
                A[i][j] = s; A[j][i] = s;
            }
            g[i] = wsum_w<W>(in ? ju[i] * ru + jv[i] * rv : 0.0);
        }
    } else {
        double Xc[3];
        cam_point(R, x + 3, X, Xc);
        const double z = fabs(Xc[2]) < 1e-12 ? 1e-12 : Xc[2];
        const double iz = 1.0 / z;                    // (the same x = X / z, y = Y / z as pose_rows_rvec: a step is judged on the residual it will be linearised at)
        ru = k.fx * (Xc[0] * iz) + k.cx - u; rv = k.fy * (Xc[1] * iz) + k.cy - v;
    }
    S = wsum_w<W>(in ? ru * ru + rv * rv : 0.0);
    rinf = wmax_w<W>(in ? fmax(fabs(ru), fabs(rv)) : 0.0);
}

// cv.solvePnPRefineLM = LMSolver::run (calib3d levmarq.cpp): D = diag(J^T J) fixed at the start, lambda_0 = 1, gain-ratio schedule
// (0.25 / 0.75, nu in [2, 10], lambda -> 0 below lambda_c), accept when the error falls, stop on |d|_inf < eps or |r|_inf < eps.
// W: the points sit in every aligned group of W lanes (cam_refine packs them when there are few: a reduction is then log2 W butterfly
// steps instead of six); W = 64 is the plain one-point-per-lane layout.
// (One copy of the loop per W in a kernel, not one per call site: a real function -- with every operand passed BY VALUE, in registers;
// through pointers the pose and the lane's point would live in scratch memory and every iteration would fetch them from there: measured,
// 2.6 -> 7.0 us per iteration on a 31-point fit.)
struct LmPose { double R[9], t[3]; };
template <int W>
__device__ __attribute__((noinline)) LmPose lm_solver_pose_fn(u64 mask, LmPose io, K4 k, double X0, double X1, double X2, double u, double v, int max_iters, double eps) {
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = io.R[i];
    t[0] = io.t[0]; t[1] = io.t[1]; t[2] = io.t[2];
    const double X[3] = {X0, X1, X2};
    double x[6];
    log_so3(R, x);
    x[3] = t[0]; x[4] = t[1]; x[5] = t[2];
    double A[6][6], g[6], S, rinf;
    pose_normal_eq<W>(mask, x, k, X, u, v, true, A, g, S, rinf);
    double D[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) D[i] = A[i][i];
    double lam = 1.0, lc = 0.75;
#ifdef SNCAL_LM_TIMING
    unsigned long long tq[5] = {0, 0, 0, 0, 0}, tp = __builtin_amdgcn_s_memtime();
#define LM_LAP(k) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); tq[k] += tn_ - tp; tp = tn_; } while (0)
#else
#define LM_LAP(k) do {} while (0)
#endif
    for (int it = 0;;) {
        double Ap[6][6], d[6], xd[6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) Ap[i][j] = A[i][j] + (i == j ? lam * D[i] : 0.0);
        {
            Chol6 F;
            chol6_factor(Ap, F);
            if (F.ok) chol6_apply(F, g, d);
            else sym_solve6(Ap, g, d);                // not positive definite: the eigen-decomposition fallback (cv::solve DECOMP_EIG)
        }
        LM_LAP(0);
#pragma unroll
        for (int i = 0; i < 6; ++i) xd[i] = x[i] - d[i];
        // (Measured and not kept: the trial evaluated WITH its normal equations, so that an accepted step is not evaluated twice -- same bits,
        // but 42 more live doubles pushed every width of this function into scratch memory: 2.97 -> 3.43 us per iteration on the 8-point
        // crawl, 3.0 -> 4.6 on a 31-point fit.)
        double A2[6][6], g2[6], Sd, rinf_d;
        RotCache rc;
        rc.valid = false;
        pose_normal_eq<W>(mask, xd, k, X, u, v, false, A2, g2, Sd, rinf_d, &rc);
        LM_LAP(1);
        double dS = 0, dv_ = 0, dmax = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double Ad = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) Ad += A[i][j] * d[j];
            dS += d[i] * (2.0 * g[i] - Ad);
            dv_ += d[i] * g[i];
            dmax = fmax(dmax, fabs(d[i]));
        }
        const double Rg = (S - Sd) / (fabs(dS) > DBL_EPS ? dS : 1.0);
        if (Rg > 0.75) {
            lam *= 0.5;
            if (lam < lc) lam = 0.0;
        } else if (Rg < 0.25) {
            double nu = (Sd - S) / (fabs(dv_) > DBL_EPS ? dv_ : 1.0) + 2.0;
            nu = fmin(fmax(nu, 2.0), 10.0);
            if (lam == 0.0) {
                double mx = DBL_EPS;
                // (lambda = 0 means the step's matrix WAS A, and keeping its factor for here would save this factorisation -- measured: no
                // gain, and the longer-lived factor pushed the function into scratch memory: 3.1 -> 4.3 us per iteration on a 31-point fit)
                Chol6 C;
                chol6_factor(A, C);
                if (C.ok) {
                    mx = fmax(mx, chol6_inv_diag_max(C));
                } else {
                    Sym6 F;                          // one factorisation for the six columns of the inverse
                    sym_factor6(A, F);
#pragma unroll
                    for (int e = 0; e < 6; ++e) {
                        double unit[6] = {0, 0, 0, 0, 0, 0}, col[6];
                        unit[e] = 1.0;
                        sym_apply6(F, unit, col);
                        mx = fmax(mx, fabs(col[e]));
                    }
                }
                lam = lc = 1.0 / mx;
                nu *= 0.5;
            }
            lam *= nu;
        }
        LM_LAP(2);
        if (Sd < S) {
#pragma unroll
            for (int i = 0; i < 6; ++i) x[i] = xd[i];
            pose_normal_eq<W>(mask, x, k, X, u, v, true, A, g, S, rinf, &rc);      // (x = xd: the rotation the trial has just built)
        }
        LM_LAP(3);
        ++it;
        if (!(it < max_iters && dmax >= eps && rinf >= eps)) {
#ifdef SNCAL_LM_TIMING
            if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) printf("LM W=%d its %d: clocks per iteration: solve %.0f trial %.0f gain+inverse %.0f accept+J %.0f\n", W, it, (double)tq[0] / it, (double)tq[1] / it, (double)tq[2] / it, (double)tq[3] / it);
#endif
            break;
        }
    }
    exp_so3(x, R);
    LmPose out;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.R[i] = R[i];
    out.t[0] = x[3]; out.t[1] = x[4]; out.t[2] = x[5];
    return out;
}
template <int W = 64>
__device__ __forceinline__ void lm_solver_pose(u64 mask, double* R, double* t, const K4& k, const double* X, double u, double v, int max_iters, double eps) {
    LmPose io;
#pragma unroll
    for (int i = 0; i < 9; ++i) io.R[i] = R[i];
    io.t[0] = t[0]; io.t[1] = t[1]; io.t[2] = t[2];
    const LmPose o = lm_solver_pose_fn<W>(mask, io, k, X[0], X[1], X[2], u, v, max_iters, eps);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = o.R[i];
    t[0] = o.t[0]; t[1] = o.t[1]; t[2] = o.t[2];
}

// lm_solver_pose with the points PACKED when there are few: point r (the r-th set bit of `mask`) goes to lane g * W + r of every aligned
// group g of W = 8 / 16 / 32 lanes, so that the 31 reductions of an iteration are 3 / 4 / 5 butterfly steps instead of 6 and every lane still
// ends with the same sums (all groups hold the same points).  The slow fits are the ill-posed ones, and those have few points (the
// bench's frame 16: 8).  More than 32 points: the plain layout.  The summation order depends on W, the results on nothing else.
template <int W>
__device__ __forceinline__ void lm_solver_pose_packed(u64 mask, int n, double* R, double* t, const K4& k, const double* X, double u, double v,
                                                      int max_iters, double eps) {
    const int lane = threadIdx.x & 63, r = lane & (W - 1);
    u64 m = mask;
    for (int i = 0; i < r; ++i) m &= m - 1;                      // (per-lane trip count, once per fit)
    const int src = (r < n && m) ? __ffsll((long long)m) - 1 : lane;
    const double Xp[3] = {__shfl(X[0], src, 64), __shfl(X[1], src, 64), __shfl(X[2], src, 64)};
    const double up = __shfl(u, src, 64), vp = __shfl(v, src, 64);
    const u64 grp = n >= 64 ? ~0ull : ((1ull << n) - 1);
    u64 pm = 0;
#pragma unroll
    for (int g = 0; g < 64 / W; ++g) pm |= grp << (g * W);
    lm_solver_pose<W>(pm, R, t, k, Xp, up, vp, max_iters, eps);
}
__device__ void lm_solver_pose_auto(u64 mask, double* R, double* t, const K4& k, const double* X, double u, double v, int max_iters, double eps) {
    const int n = popc64(mask);
    if (n >= 1 && n <= 8) lm_solver_pose_packed<8>(mask, n, R, t, k, X, u, v, max_iters, eps);
    else if (n <= 16 && n >= 1) lm_solver_pose_packed<16>(mask, n, R, t, k, X, u, v, max_iters, eps);
    else if (n <= 32 && n >= 1) lm_solver_pose_packed<32>(mask, n, R, t, k, X, u, v, max_iters, eps);
    else lm_solver_pose<64>(mask, R, t, k, X, u, v, max_iters, eps);
}

// cvFindExtrinsicCameraParams2's refinement (solvePnPRansac's final SOLVEPNP_ITERATIVE refit, calibrateCamera's per-view initial
// extrinsics): CvLevMarq over [rvec, tvec] -- lambda = 10^k, k_0 = -3, diagonal x (1 + lambda), steps from the same normal equations
// until the error no longer grows (k + 1 per rejection, up to 16), an accepted step lowers k; criteria (max_iter, eps on |dx| / |x|)
__device__ void cvlevmarq_pose(u64 mask, double* R, double* t, const K4& k, const double* X, double u, double v, int max_iter, double eps) {
    double x[6];
    log_so3(R, x);
    x[3] = t[0]; x[4] = t[1]; x[5] = t[2];
    double A[6][6], g[6], e_prev, rinf;
    pose_normal_eq(mask, x, k, X, u, v, true, A, g, e_prev, rinf);
    int kk = -3, iters = 0;
    for (;;) {
        double cand[6], e = INFINITY;
        bool have = false;
        for (;;) {
            const double lam = pow(10.0, (double)kk);
            double Ad[6][6], d[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) Ad[i][j] = A[i][j] + (i == j ? lam * A[i][i] : 0.0);
            sym_solve6(Ad, g, d);                               // cv::solve(..., DECOMP_SVD): a step even when not positive definite
            {
#pragma unroll
                for (int i = 0; i < 6; ++i) cand[i] = x[i] - d[i];
                double A2[6][6], g2[6], r2;
                pose_normal_eq(mask, cand, k, X, u, v, false, A2, g2, e, r2);
                have = true;
            }
            if (!(e > e_prev)) break;
            if (++kk > 16) break;
        }
        if (!have || !isfinite(e)) break;                    // no usable step at any damping: keep the last parameters
        kk = max(kk - 1, -16);
        double dn = 0, pn = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { dn += (cand[i] - x[i]) * (cand[i] - x[i]); pn += x[i] * x[i]; x[i] = cand[i]; }
        ++iters;
        if (iters >= max_iter || sqrt(dn) / fmax(sqrt(pn), 1e-300) < eps) break;
        pose_normal_eq(mask, x, k, X, u, v, true, A, g, e_prev, rinf);
    }
    exp_so3(x, R);
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
}

__device__ __forceinline__ void refit_pose(int sched, u64 mask, double* R, double* t, const K4& k, const double* X, double u, double v) {
    if (sched == SCHED_OPENCV) cvlevmarq_pose(mask, R, t, k, X, u, v, 20, FLT_EPS);
    else refine_pose_lm(mask, R, t, k, X, u, v, 20, 1e-10);
}

// Lane-local damped Gauss-Newton polish of a minimal-sample pose on its own 4 (z=0) points.  The closed-form
// homography decomposition is badly conditioned for long focal lengths; a few iterations repair it.
__device__ void polish4(double* R, double* t, const K4& k, const double (&s)[4][2], const double (&d)[4][2]) {
    auto cost = [&](const double* R_, const double* t_) {
        double c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double Xq[3] = {s[q][0], s[q][1], 0.0};
            double z;
            c += reproj_e2(R_, t_, k, Xq, d[q][0], d[q][1], &z);
        }
        return c;
    };
    double c0 = cost(R, t);
    for (int it = 0; it < 8; ++it) {
        double A[6][6], g[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) { g[i] = 0; for (int j = 0; j < 6; ++j) A[i][j] = 0; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double Xq[3] = {s[q][0], s[q][1], 0.0};
            double ju[6], jv[6], ru, rv, xn, yn;
            pose_rows(R, t, k.fx, k.fy, k.cx, k.cy, Xq, d[q][0], d[q][1], ju, jv, ru, rv, xn, yn);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 6; ++j) A[i][j] += ju[i] * ju[j] + jv[i] * jv[j];
                g[i] -= ju[i] * ru + jv[i] * rv;
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i][i] += 1e-3 * A[i][i];
        double step[6] = {0, 0, 0, 0, 0, 0}, Rn[9], tn[3];
        if (!chol_solve<6>(A, g, step)) break;
        apply_step(R, t, step, Rn, tn);
        const double c1 = cost(Rn, tn);
        if (!(c1 < c0)) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        t[0] = tn[0]; t[1] = tn[1]; t[2] = tn[2];
        c0 = c1;
    }
}

// Camera.solve_pnp (camera.py:92-103): planar minimal solver on the z=0 points (64 lane-parallel 4-point
// hypotheses + one least-squares homography over all of them), 8 px inliers, LM refit on the inliers
__device__ bool pnp_ransac(int sched, u64 mask, u64 gmask, const K4& k, const double* X, double u, double v, double* R, double* t) {
    const int lane = threadIdx.x & 63;
    const int n = popc64(gmask);
    if (n < 4) return false;
    int idx[4] = {0, 0, 0, 0};
    bool ok = sample4(lane, n, idx);
    double s[4][2], d[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int src = kth_set_bit(gmask, idx[q]);
        s[q][0] = __shfl(X[0], src, 64); s[q][1] = __shfl(X[1], src, 64);
        d[q][0] = __shfl(u, src, 64); d[q][1] = __shfl(v, src, 64);
    }
    double Hh[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Rh[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, th[3] = {0, 0, 1};
    ok = ok && homography_4pt(s, d, Hh);
    ok = ok && pose_from_homography(Hh, k.fx, k.fy, k.cx, k.cy, Rh, th);
    if (ok) polish4(Rh, th, k, s, d);
    int cnt = 0;
    double se = 0;
    for (u64 m = mask; m; m &= m - 1) {
        const int j = __ffsll((long long)m) - 1;
        const double Xj[3] = {bcast(X[0], j), bcast(X[1], j), bcast(X[2], j)};
        const double uj = bcast(u, j), vj = bcast(v, j);
        if (ok) {
            double z;
            const double e2 = reproj_e2(Rh, th, k, Xj, uj, vj, &z);
            if (e2 <= 64.0 && z > 1e-9) { ++cnt; se += e2; }
        }
    }
    const Best best = wave_best(Best{ok ? cnt : -1, ok ? se : INFINITY, lane});
    int best_cnt = best.cnt;
    if (best.cnt >= 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = bcast(Rh[i], best.h);
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = bcast(th[i], best.h);
    }
    {   // hypothesis NH_PNP: least-squares homography over every z=0 point (stable when a 4-point sample is not)
        double Hl[9], Rl[9], tl[3];
        if (homography_lsq(gmask, X[0], X[1], u, v, 10, Hl) && pose_from_homography(Hl, k.fx, k.fy, k.cx, k.cy, Rl, tl)) {
            refit_pose(sched, gmask, Rl, tl, k, X, u, v);
            double z;
            const double e2 = reproj_e2(Rl, tl, k, X, u, v, &z);
            const bool inl = ((mask >> lane) & 1) && e2 <= 64.0 && z > 1e-9;
            const int c2 = popc64(__ballot(inl));
            const double s2 = wsum(inl ? e2 : 0.0);
            if (c2 > best_cnt || (c2 == best_cnt && s2 < best.s)) {
                best_cnt = c2;
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = Rl[i];
                t[0] = tl[0]; t[1] = tl[1]; t[2] = tl[2];
            }
        }
    }
    if (best_cnt < 4) return false;
    double z;
    const double e2 = reproj_e2(R, t, k, X, u, v, &z);
    const u64 inl = __ballot(((mask >> lane) & 1) && e2 <= 64.0 && z > 1e-9);
    refit_pose(sched, inl, R, t, k, X, u, v);
    return true;
}

}  // namespace
