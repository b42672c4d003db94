// Part of the camera solve: included by solve.hip and by labels.hip (one translation unit each), after solve_wave.hpp.
// Lane-local dense algebra: 3x3 products and adjugates, NxN Cholesky, the polar iteration, the SO(3) maps (exp, log, left Jacobian)
// and the two 6x6 solvers of the pose minimisers (Sym6: Cholesky with the eigen-decomposition fallback; Chol6: reciprocal-diagonal form).
#pragma once

namespace {

// ---- small dense algebra (register resident, fully unrolled) -------------------------------------------
__device__ __forceinline__ double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__device__ __forceinline__ void adj3(const double* m, double* a) {   // adjugate: inv = adj / det
    a[0] = m[4] * m[8] - m[5] * m[7]; a[1] = m[2] * m[7] - m[1] * m[8]; a[2] = m[1] * m[5] - m[2] * m[4];
    a[3] = m[5] * m[6] - m[3] * m[8]; a[4] = m[0] * m[8] - m[2] * m[6]; a[5] = m[2] * m[3] - m[0] * m[5];
    a[6] = m[3] * m[7] - m[4] * m[6]; a[7] = m[1] * m[6] - m[0] * m[7]; a[8] = m[0] * m[4] - m[1] * m[3];
}
__device__ __forceinline__ void mul33(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}
__device__ __forceinline__ void mul3v(const double* a, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = a[i * 3] * v[0] + a[i * 3 + 1] * v[1] + a[i * 3 + 2] * v[2];
}

// SPD solve by Cholesky on a packed-full NxN matrix; false when a pivot <= rel_tol * max diag
template <int N>
__device__ __forceinline__ bool chol_solve(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
    double L[N][N];
    double dmax = A[0][0];
#pragma unroll
    for (int i = 1; i < N; ++i) dmax = fmax(dmax, A[i][i]);
    if (!(dmax > 0)) return false;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 1e-11 * dmax)) { ok = false; d = 1.0; }
        const double ljj = sqrt(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    if (!ok) return false;
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
    return true;
}

__device__ __forceinline__ void polar3(double* R) {   // nearest rotation by Newton iteration
    if (det3(R) < 0) { R[2] = -R[2]; R[5] = -R[5]; R[8] = -R[8]; }
    for (int it = 0; it < 12; ++it) {
        double a[9];
        adj3(R, a);
        const double d = det3(R);
        // inv(R)^T = adj^T / det
        const double n[9] = {a[0] / d, a[3] / d, a[6] / d, a[1] / d, a[4] / d, a[7] / d, a[2] / d, a[5] / d, a[8] / d};
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = 0.5 * (R[i] + n[i]);
    }
}

__device__ __forceinline__ void exp_so3(const double* w, double* E) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    mul33(K, K, K2);
    double a, b;
    if (th < 1e-8) { a = 1.0; b = 0.5; }
    else { a = sin(th) / th; b = (1 - cos(th)) / (th * th); }
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

constexpr double FLT_EPS = 1.1920928955078125e-07, DBL_EPS = 2.220446049250313e-16;

__device__ __forceinline__ void log_so3(const double* R, double* r) {       // cv.Rodrigues(matrix -> vector), R orthonormal
    const double c = fmin(1.0, fmax(-1.0, (R[0] + R[4] + R[8] - 1.0) * 0.5));
    const double th = acos(c);
    const double a[3] = {(R[7] - R[5]) * 0.5, (R[2] - R[6]) * 0.5, (R[3] - R[1]) * 0.5};      // sin(th) * axis
    const double sn = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    if (sn < 1e-5) {
        if (c > 0) { r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; return; }
        // th ~ pi: axis from the symmetric part (R + I) / 2 = axis axis^T, sign from what is left of the antisymmetric part
        const double B[9] = {(R[0] + 1) * 0.5, R[1] * 0.5, R[2] * 0.5, R[3] * 0.5, (R[4] + 1) * 0.5, R[5] * 0.5, R[6] * 0.5, R[7] * 0.5, (R[8] + 1) * 0.5};
        const double d0 = sqrt(fmax(B[0], 0.0)), d1 = sqrt(fmax(B[4], 0.0)), d2 = sqrt(fmax(B[8], 0.0));
        const int kx = d0 >= d1 && d0 >= d2 ? 0 : (d1 >= d2 ? 1 : 2);
        const double dk = fmax(kx == 0 ? d0 : kx == 1 ? d1 : d2, 1e-300);
        double ax[3] = {B[kx] / dk, B[3 + kx] / dk, B[6 + kx] / dk};
        const double n = fmax(sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), 1e-300);
        const double sg = (a[0] * ax[0] + a[1] * ax[1] + a[2] * ax[2]) < 0 ? -1.0 : 1.0;
        r[0] = sg * ax[0] / n * th; r[1] = sg * ax[1] / n * th; r[2] = sg * ax[2] / n * th;
        return;
    }
    const double q = th / sn;
    r[0] = a[0] * q; r[1] = a[1] * q; r[2] = a[2] * q;
}

// The two maps of a rotation vector with the angle and its sine / cosine given (ONE sincos for both, pose_normal_eq): the same
// formulas as exp_so3 / left_jacobian_so3
struct RotAngle { double th, sn, cs; };
__device__ __forceinline__ RotAngle rot_angle(const double* w) {
    RotAngle a;
    a.th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    sincos(a.th, &a.sn, &a.cs);
    return a;
}
__device__ __forceinline__ void exp_so3_a(const double* w, const RotAngle& q, double* E) {
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    mul33(K, K, K2);
    double a, b;
    if (q.th < 1e-8) { a = 1.0; b = 0.5; }
    else { a = q.sn / q.th; b = (1 - q.cs) / (q.th * q.th); }
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}
__device__ __forceinline__ void left_jacobian_so3_a(const double* w, const RotAngle& q, double* J) {
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    mul33(K, K, K2);
    double a, b;
    if (q.th < 1e-6) { a = 0.5; b = 1.0 / 6.0; }
    else { a = (1 - q.cs) / (q.th * q.th); b = (q.th - q.sn) / (q.th * q.th * q.th); }
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

// exp(r + d) ~ exp(J_l(r) d) exp(r)
__device__ __forceinline__ void left_jacobian_so3(const double* w, double* J) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double K2[9];
    mul33(K, K, K2);
    double a, b;
    if (th < 1e-6) { a = 0.5; b = 1.0 / 6.0; }
    else { a = (1 - cos(th)) / (th * th); b = (th - sin(th)) / (th * th * th); }
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * K[i] + b * K2[i];
}

// cv::solve(A, b, DECOMP_EIG / DECOMP_SVD) for a symmetric 6x6 system: Cholesky when A is positive definite, else the minimum-norm
// solution from a cyclic Jacobi eigen-decomposition with eigenvalues below 2 eps sum|w| dropped
// (The rotation indices are compile-time constants -- fully unrolled pair loop -- so that M and V live in registers: with run-time
// indices they sat in scratch memory and one fallback solve cost tens of thousands of clocks; the slow LM runs of degenerate
// candidates are exactly the ones that take this path every iteration.  Same operations in the same order as before.)
struct Sym6 { bool chol; double L[6][6]; double M[6][6], V[6][6]; double thr; };
__device__ __forceinline__ void sym_factor6(const double (&A)[6][6], Sym6& F) {
    // Cholesky factor (chol_solve's): usable when every pivot passes
    double dmax = A[0][0];
#pragma unroll
    for (int i = 1; i < 6; ++i) dmax = fmax(dmax, A[i][i]);
    bool ok = dmax > 0;
    if (ok) {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double d = A[j][j];
#pragma unroll
            for (int k = 0; k < j; ++k) d -= F.L[j][k] * F.L[j][k];
            if (!(d > 1e-11 * dmax)) { ok = false; d = 1.0; }
            const double ljj = sqrt(d);
            F.L[j][j] = ljj;
#pragma unroll
            for (int i = j + 1; i < 6; ++i) {
                double s = A[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) s -= F.L[i][k] * F.L[j][k];
                F.L[i][j] = s / ljj;
            }
        }
    }
    F.chol = ok;
    if (ok) return;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { F.M[i][j] = A[i][j]; F.V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 12; ++sweep) {
        double off = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i + 1; j < 6; ++j) off += F.M[i][j] * F.M[i][j];
        if (!(off > 1e-300)) break;
#pragma unroll
        for (int p_ = 0; p_ < 5; ++p_)
#pragma unroll
            for (int q_ = p_ + 1; q_ < 6; ++q_) {
                const double apq = F.M[p_][q_];
                if (apq != 0.0) {
                    const double th = (F.M[q_][q_] - F.M[p_][p_]) / (2.0 * apq);
                    const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
#pragma unroll
                    for (int k2 = 0; k2 < 6; ++k2) { const double a = F.M[k2][p_], bb = F.M[k2][q_]; F.M[k2][p_] = cs * a - sn * bb; F.M[k2][q_] = sn * a + cs * bb; }
#pragma unroll
                    for (int k2 = 0; k2 < 6; ++k2) { const double a = F.M[p_][k2], bb = F.M[q_][k2]; F.M[p_][k2] = cs * a - sn * bb; F.M[q_][k2] = sn * a + cs * bb; }
#pragma unroll
                    for (int k2 = 0; k2 < 6; ++k2) { const double a = F.V[k2][p_], bb = F.V[k2][q_]; F.V[k2][p_] = cs * a - sn * bb; F.V[k2][q_] = sn * a + cs * bb; }
                }
            }
    }
    double sw = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) sw += fabs(F.M[i][i]);
    F.thr = 2.0 * DBL_EPS * sw;
}
__device__ __forceinline__ void sym_apply6(const Sym6& F, const double (&b)[6], double (&x)[6]) {
    if (F.chol) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double s = b[i];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= F.L[i][k] * y[k];
            y[i] = s / F.L[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double s = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) s -= F.L[k][i] * x[k];
            x[i] = s / F.L[i][i];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = 0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        if (!(fabs(F.M[e][e]) > F.thr)) continue;
        double pj = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) pj += F.V[i][e] * b[i];
        pj /= F.M[e][e];
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] += F.V[i][e] * pj;
    }
}
__device__ void sym_solve6(const double (&A)[6][6], const double (&b)[6], double (&x)[6]) {
    Sym6 F;
    sym_factor6(A, F);
    sym_apply6(F, b, x);
}

// Cholesky of a 6 x 6 system for the LM below, with the diagonal kept as RECIPROCALS: L[i][j] = s * rinv[j] and the substitutions
// multiply -- 6 reciprocal square roots per factorisation and no division in a solve, where chol_solve's form has 6 square roots + 15
// divisions per factorisation and 12 dependent divisions per solve.  refine_camera's slow fits (20000 iterations at the reference's
// criterion, camera.py:116) are ONE wavefront issuing ~2200 dependent fp64 instructions per iteration: 7.8 us each, 160 ms for the fit that
// sets the latency of a batch's solve (NOTES/design_history_r1_r5.md §11.1); a fifth of those instructions were divisions.  Same pivot rule as sym_factor6 (a
// failing pivot sends the caller to its eigen-decomposition fallback); results differ from the dividing form by rounding only.
struct Chol6 { double L[6][6]; double rinv[6]; bool ok; };
__device__ __forceinline__ void chol6_factor(const double (&A)[6][6], Chol6& F) {
    double dmax = A[0][0];
#pragma unroll
    for (int i = 1; i < 6; ++i) dmax = fmax(dmax, A[i][i]);
    bool ok = dmax > 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= F.L[j][k] * F.L[j][k];
        if (!(d > 1e-11 * dmax)) { ok = false; d = 1.0; }
        const double ri = rsqrt(d);
        F.rinv[j] = ri;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double sacc = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) sacc -= F.L[i][k] * F.L[j][k];
            F.L[i][j] = sacc * ri;
        }
    }
    F.ok = ok;
}
__device__ __forceinline__ void chol6_apply(const Chol6& F, const double (&b)[6], double (&x)[6]) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double sacc = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) sacc -= F.L[i][k] * y[k];
        y[i] = sacc * F.rinv[i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double sacc = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) sacc -= F.L[k][i] * x[k];
        x[i] = sacc * F.rinv[i];
    }
}
// max_e |(A^-1)_ee| from the factor: A^-1 = L^-T L^-1, so (A^-1)_ee = sum_i (L^-1)_ie^2 -- column e of L^-1 by one forward
// substitution of a unit vector, instead of six full solves
__device__ __forceinline__ double chol6_inv_diag_max(const Chol6& F) {
    double mx = 0;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
        double z[6], acc = 0;
#pragma unroll
        for (int i = e; i < 6; ++i) {
            double sacc = i == e ? 1.0 : 0.0;
#pragma unroll
            for (int k = e; k < i; ++k) sacc -= F.L[i][k] * z[k];
            z[i] = sacc * F.rinv[i];
            acc += z[i] * z[i];
        }
        mx = fmax(mx, acc);
    }
    return mx;
}

}  // namespace
