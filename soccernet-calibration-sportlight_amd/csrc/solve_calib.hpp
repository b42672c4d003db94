// Part of the camera solve: included by solve.hip alone (one translation unit), after solve_pose.hpp.
// One focal length and the per-view poses from one to three planar views of the pitch (ground plane, the two goal planes).
#pragma once

namespace {

// ---- calibrateCamera restatement (planar views, pp fixed at ((w-1)/2,(h-1)/2), aspect 1, no distortion) ----
struct View { u64 mask; int kind; double weight; };   // kind 0 ground (x,y), 1 goal plane (y,z)

__device__ bool calibrate_planes(int sched, const View* views, int nviews, const double* X32, double u32, double v32, int img_w,
                                 int img_h, double& f_out, double* R0, double* t0) {
    const int lane = threadIdx.x & 63;
    const double cx = (img_w - 1) * 0.5, cy = (img_h - 1) * 0.5;
    double Hs[3][9];
    double n00 = 0, n01 = 0, n11 = 0, r0 = 0, r1 = 0;
    for (int vi = 0; vi < nviews; ++vi) {
        const double px = views[vi].kind ? X32[1] : X32[0], py = views[vi].kind ? X32[2] : X32[1];
        if (!homography_lsq(views[vi].mask, px, py, u32, v32, 10, Hs[vi])) return false;
        double Hc[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Hc[i] = Hs[vi][i];
        Hc[0] -= Hc[6] * cx; Hc[1] -= Hc[7] * cx; Hc[2] -= Hc[8] * cx;
        Hc[3] -= Hc[6] * cy; Hc[4] -= Hc[7] * cy; Hc[5] -= Hc[8] * cy;
        double h[3] = {Hc[0], Hc[3], Hc[6]}, v[3] = {Hc[1], Hc[4], Hc[7]}, d1[3], d2[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { d1[i] = (h[i] + v[i]) * 0.5; d2[i] = (h[i] - v[i]) * 0.5; }
        auto nrm = [](double* a) {
            const double n = fmax(sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), 1e-300);
            a[0] /= n; a[1] /= n; a[2] /= n;
        };
        nrm(h); nrm(v); nrm(d1); nrm(d2);
        const double sw = sqrt(views[vi].weight);
        const double a0[2] = {sw * (h[0] * v[0]), sw * (h[1] * v[1])}, b0 = -sw * h[2] * v[2];
        const double a1[2] = {sw * (d1[0] * d2[0]), sw * (d1[1] * d2[1])}, b1 = -sw * d1[2] * d2[2];
        n00 += a0[0] * a0[0] + a1[0] * a1[0]; n01 += a0[0] * a0[1] + a1[0] * a1[1]; n11 += a0[1] * a0[1] + a1[1] * a1[1];
        r0 += a0[0] * b0 + a1[0] * b1; r1 += a0[1] * b0 + a1[1] * b1;
    }
    const double det = n00 * n11 - n01 * n01;
    if (!(fabs(det) > 1e-14 * fmax(n00 * n11, 1e-300))) return false;
    const double s0 = (n11 * r0 - n01 * r1) / det, s1 = (n00 * r1 - n01 * r0) / det;
    if (s0 == 0 || s1 == 0) return false;
    double f = 0.5 * (sqrt(fabs(1.0 / s0)) + sqrt(fabs(1.0 / s1)));
    if (!isfinite(f) || f <= 0) return false;
    double Rv[3][9], tv[3][3];
    for (int vi = 0; vi < nviews; ++vi) {
        if (!pose_from_homography(Hs[vi], f, f, cx, cy, Rv[vi], tv[vi])) return false;
        const double Xp[3] = {views[vi].kind ? X32[1] : X32[0], views[vi].kind ? X32[2] : X32[1], 0.0};
        const K4 k{f, f, cx, cy};
        refit_pose(sched, views[vi].mask, Rv[vi], tv[vi], k, Xp, u32, v32);
    }
    if (sched == SCHED_OPENCV) {
        // calibrateCamera's joint fit (cvCalibrateCamera2Internal, CvLevMarq::updateAlt, criteria (30, DBL_EPSILON)): free parameters
        // fy (fx slaved) and [rvec, tvec] per view; duplicated views (Q1) are weights; block-arrowhead normal equations through the
        // Schur complement on f (= OpenCV's dense SVD solve whenever the pose blocks are non-singular)
        double xs[3][6];
        for (int vi = 0; vi < nviews; ++vi) {
            log_so3(Rv[vi], xs[vi]);
            xs[vi][3] = tv[vi][0]; xs[vi][4] = tv[vi][1]; xs[vi][5] = tv[vi][2];
        }
        double A[3][6][6], Bv[3][6], g[3][6], aff = 0, gf = 0;
        auto evaluate = [&](double f_, const double (*xx)[6], bool want_j) -> double {
            if (!(f_ > 0)) return INFINITY;
            double err = 0;
            if (want_j) { aff = 0; gf = 0; }
            for (int vi = 0; vi < nviews; ++vi) {
                const bool in = (views[vi].mask >> lane) & 1;
                const double Xp[3] = {views[vi].kind ? X32[1] : X32[0], views[vi].kind ? X32[2] : X32[1], 0.0};
                double Rr[9], Jl[9], ju[6], jv[6], ru, rv, xn, yn;
                exp_so3(xx[vi], Rr);
                left_jacobian_so3(xx[vi], Jl);
                pose_rows_rvec(Rr, Jl, xx[vi] + 3, f_, f_, cx, cy, Xp, u32, v32, ju, jv, ru, rv, xn, yn);
                const double wgt = views[vi].weight;
                err += wgt * wsum(in ? ru * ru + rv * rv : 0.0);
                if (want_j) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
#pragma unroll
                        for (int j = i; j < 6; ++j) {
                            const double s2 = wgt * wsum(in ? ju[i] * ju[j] + jv[i] * jv[j] : 0.0);
                            A[vi][i][j] = s2; A[vi][j][i] = s2;
                        }
                        Bv[vi][i] = wgt * wsum(in ? ju[i] * xn + jv[i] * yn : 0.0);
                        g[vi][i] = wgt * wsum(in ? ju[i] * ru + jv[i] * rv : 0.0);
                    }
                    aff += wgt * wsum(in ? xn * xn + yn * yn : 0.0);
                    gf += wgt * wsum(in ? xn * ru + yn * rv : 0.0);
                }
            }
            return err;
        };
        double e_prev = evaluate(f, xs, true);
        int kk = -3, iters = 0;
        for (;;) {
            double fc = f, xc[3][6], e = INFINITY;
            bool have = false;
            for (;;) {
                const double lam = pow(10.0, (double)kk);
                double s_aff = aff * (1 + lam), s_g = gf, AiB[3][6], Aig[3][6];
                bool ok = true;
                for (int vi = 0; vi < nviews && ok; ++vi) {
                    double Ad[6][6];
#pragma unroll
                    for (int i = 0; i < 6; ++i)
#pragma unroll
                        for (int j = 0; j < 6; ++j) Ad[i][j] = A[vi][i][j] + (i == j ? lam * A[vi][i][i] : 0.0);
                    // (OpenCV: one dense cv::solve(DECOMP_SVD); a pose block that is not positive definite never aborts the step)
                    sym_solve6(Ad, Bv[vi], AiB[vi]);
                    sym_solve6(Ad, g[vi], Aig[vi]);
#pragma unroll
                    for (int i = 0; i < 6; ++i) { s_aff -= Bv[vi][i] * AiB[vi][i]; s_g -= Bv[vi][i] * Aig[vi][i]; }
                }
                have = ok && !(fabs(s_aff) < 1e-300);
                if (have) {
                    const double df = s_g / s_aff;                  // x' = x - d
                    fc = f - df;
                    for (int vi = 0; vi < nviews; ++vi)
#pragma unroll
                        for (int i = 0; i < 6; ++i) xc[vi][i] = xs[vi][i] - (Aig[vi][i] - AiB[vi][i] * df);
                    e = evaluate(fc, xc, false);
                } else e = INFINITY;
                if (!(e > e_prev)) break;
                if (++kk > 16) break;
            }
            if (!have || !isfinite(e)) break;
            kk = max(kk - 1, -16);
            double dn = (fc - f) * (fc - f), pn = f * f;
            for (int vi = 0; vi < nviews; ++vi)
#pragma unroll
                for (int i = 0; i < 6; ++i) { dn += views[vi].weight * (xc[vi][i] - xs[vi][i]) * (xc[vi][i] - xs[vi][i]); pn += views[vi].weight * xs[vi][i] * xs[vi][i]; xs[vi][i] = xc[vi][i]; }
            f = fc;
            ++iters;
            if (iters >= 30 || sqrt(dn) / fmax(sqrt(pn), 1e-300) < DBL_EPS) break;
            e_prev = evaluate(f, xs, true);
        }
        if (!isfinite(f) || f <= 0) return false;
        f_out = f;
        exp_so3(xs[0], R0);
        polar3(R0);
        t0[0] = xs[0][3]; t0[1] = xs[0][4]; t0[2] = xs[0][5];
        return true;
    }
    auto total_cost = [&](double f_, double (*Rs)[9], double (*ts)[3]) {
        double c = 0;
        for (int vi = 0; vi < nviews; ++vi) {
            const double Xp[3] = {views[vi].kind ? X32[1] : X32[0], views[vi].kind ? X32[2] : X32[1], 0.0};
            const K4 k{f_, f_, cx, cy};
            double z;
            const double e2 = reproj_e2(Rs[vi], ts[vi], k, Xp, u32, v32, &z);
            c += views[vi].weight * wsum(((views[vi].mask >> lane) & 1) ? e2 : 0.0);
        }
        return c;
    };
    double lam = 1e-3;
    double c0 = total_cost(f, Rv, tv);
    for (int it = 0; it < 60; ++it) {
        double A[3][6][6], Bv[3][6], g[3][6];
        double aff = 0, gf = 0;
        for (int vi = 0; vi < nviews; ++vi) {
            const bool in = (views[vi].mask >> lane) & 1;
            const double Xp[3] = {views[vi].kind ? X32[1] : X32[0], views[vi].kind ? X32[2] : X32[1], 0.0};
            double ju[6], jv[6], ru, rv, xn, yn;
            pose_rows(Rv[vi], tv[vi], f, f, cx, cy, Xp, u32, v32, ju, jv, ru, rv, xn, yn);
            const double wgt = views[vi].weight;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    const double s = wgt * wsum(in ? ju[i] * ju[j] + jv[i] * jv[j] : 0.0);
                    A[vi][i][j] = s; A[vi][j][i] = s;
                }
                Bv[vi][i] = wgt * wsum(in ? ju[i] * xn + jv[i] * yn : 0.0);
                g[vi][i] = wgt * wsum(in ? ju[i] * ru + jv[i] * rv : 0.0);
            }
            aff += wgt * wsum(in ? xn * xn + yn * yn : 0.0);
            gf += wgt * wsum(in ? xn * ru + yn * rv : 0.0);
        }
        bool improved = false;
        double dc = 0;
        for (int tr = 0; tr < 12; ++tr) {
            double s_aff = aff * (1 + lam), s_g = gf;
            double AiB[3][6], Aig[3][6];
            bool ok = true;
            for (int vi = 0; vi < nviews && ok; ++vi) {
                double Ad[6][6];
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = 0; j < 6; ++j) Ad[i][j] = A[vi][i][j] + (i == j ? lam * A[vi][i][i] : 0.0);
                ok = chol_solve<6>(Ad, Bv[vi], AiB[vi]) && chol_solve<6>(Ad, g[vi], Aig[vi]);
                if (ok) {
#pragma unroll
                    for (int i = 0; i < 6; ++i) { s_aff -= Bv[vi][i] * AiB[vi][i]; s_g -= Bv[vi][i] * Aig[vi][i]; }
                }
            }
            if (!ok || fabs(s_aff) < 1e-300) { lam *= 10; continue; }
            const double df = -s_g / s_aff;
            double Rn[3][9], tn[3][3];
            for (int vi = 0; vi < nviews; ++vi) {
                double step[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) step[i] = -(Aig[vi][i] + AiB[vi][i] * df);
                apply_step(Rv[vi], tv[vi], step, Rn[vi], tn[vi]);
            }
            const double fn = f + df;
            const double c1 = fn > 0 ? total_cost(fn, Rn, tn) : INFINITY;
            if (c1 < c0) {
                dc = c0 - c1; c0 = c1; f = fn;
                for (int vi = 0; vi < nviews; ++vi) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) Rv[vi][i] = Rn[vi][i];
                    tv[vi][0] = tn[vi][0]; tv[vi][1] = tn[vi][1]; tv[vi][2] = tn[vi][2];
                }
                lam = fmax(lam * 0.1, 1e-15);
                improved = true;
                break;
            }
            lam *= 10;
        }
        if (!improved || dc <= 1e-16 * fmax(c0, 1e-30)) break;
    }
    f_out = f;
#pragma unroll
    for (int i = 0; i < 9; ++i) R0[i] = Rv[0][i];
    polar3(R0);
    t0[0] = tv[0][0]; t0[1] = tv[0][1]; t0[2] = tv[0][2];
    return true;
}

}  // namespace
