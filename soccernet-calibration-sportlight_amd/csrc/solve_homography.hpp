// Part of the camera solve: included by solve.hip and by labels.hip (one translation unit each), after solve_wave.hpp and
// solve_linalg.hpp.
// Plane homographies: the 4-point fit, the normalised least-squares fit, RANSAC over lane-parallel hypotheses, and the focal length
// from the image of the absolute conic.
#pragma once

namespace {

// ---- homography ----------------------------------------------------------------------------------
__device__ __forceinline__ bool basis_map(const double (&p)[4][2], double* out) {
    const double M[9] = {p[0][0], p[1][0], p[2][0], p[0][1], p[1][1], p[2][1], 1.0, 1.0, 1.0};
    const double det = det3(M);
    double mx = 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmax(mx, fmax(fabs(p[i][0]), fabs(p[i][1])));
    if (fabs(det) < 1e-9 * mx * mx) return false;
    double a[9];
    adj3(M, a);
    const double rhs[3] = {p[3][0], p[3][1], 1.0};
    double lam[3];
    mul3v(a, rhs, lam);
    lam[0] /= det; lam[1] /= det; lam[2] /= det;
    if (fmin(fabs(lam[0]), fmin(fabs(lam[1]), fabs(lam[2]))) < 1e-9) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = M[i * 3 + j] * lam[j];
    return true;
}

__device__ __forceinline__ bool homography_4pt(const double (&s)[4][2], const double (&d)[4][2], double* H) {
    double A[9], B[9];
    if (!basis_map(s, A) || !basis_map(d, B)) return false;
    const double detA = det3(A);
    if (fabs(detA) < 1e-300) return false;
    double adjA[9];
    adj3(A, adjA);
#pragma unroll
    for (int i = 0; i < 9; ++i) adjA[i] /= detA;
    mul33(B, adjA, H);
    if (fabs(H[8]) < 1e-12) return false;
    const double s8 = H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] /= s8;
    return true;
}

__device__ __forceinline__ void apply_h(const double* H, double x, double y, double& u, double& v) {
    double w = H[6] * x + H[7] * y + H[8];
    if (fabs(w) < 1e-300) w = 1e-300;
    u = (H[0] * x + H[1] * y + H[2]) / w;
    v = (H[3] * x + H[4] * y + H[5]) / w;
}

// normalised least squares (h33 = 1) + `iters` damped Gauss-Newton steps on the reprojection error
__device__ bool homography_lsq(u64 mask, double sx, double sy, double du, double dv, int iters, double* H) {
    const int lane = threadIdx.x & 63;
    const bool in = (mask >> lane) & 1;
    const double n = (double)popc64(mask);
    const double csx = wsum(in ? sx : 0.0) / n, csy = wsum(in ? sy : 0.0) / n;
    const double cdx = wsum(in ? du : 0.0) / n, cdy = wsum(in ? dv : 0.0) / n;
    const double ms = wsum(in ? sqrt((sx - csx) * (sx - csx) + (sy - csy) * (sy - csy)) : 0.0) / n;
    const double md = wsum(in ? sqrt((du - cdx) * (du - cdx) + (dv - cdy) * (dv - cdy)) : 0.0) / n;
    const double ss = sqrt(2.0) / fmax(ms, 1e-12), sd = sqrt(2.0) / fmax(md, 1e-12);
    const double x = (sx - csx) * ss, y = (sy - csy) * ss, u = (du - cdx) * sd, v = (dv - cdy) * sd;
    double A[8][8], b[8], h[8];
    {
        const double ru[8] = {x, y, 1, 0, 0, 0, -u * x, -u * y};
        const double rv[8] = {0, 0, 0, x, y, 1, -v * x, -v * y};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = i; j < 8; ++j) {
                const double s = wsum(in ? ru[i] * ru[j] + rv[i] * rv[j] : 0.0);
                A[i][j] = s; A[j][i] = s;
            }
            b[i] = wsum(in ? ru[i] * u + rv[i] * v : 0.0);
        }
    }
    if (!chol_solve<8>(A, b, h)) return false;
    auto cost = [&](const double* hh) {
        double w = hh[6] * x + hh[7] * y + 1.0;
        if (fabs(w) < 1e-300) w = 1e-300;
        const double pu = (hh[0] * x + hh[1] * y + hh[2]) / w - u, pv = (hh[3] * x + hh[4] * y + hh[5]) / w - v;
        return wsum(in ? pu * pu + pv * pv : 0.0);
    };
    double lam = 1e-3;
    double c0 = cost(h);
    for (int it = 0; it < iters; ++it) {
        const double w = h[6] * x + h[7] * y + 1.0;
        const double pu = (h[0] * x + h[1] * y + h[2]) / w, pv = (h[3] * x + h[4] * y + h[5]) / w;
        const double ju[8] = {x / w, y / w, 1 / w, 0, 0, 0, -pu * x / w, -pu * y / w};
        const double jv[8] = {0, 0, 0, x / w, y / w, 1 / w, -pv * x / w, -pv * y / w};
        const double eu = pu - u, ev = pv - v;
        double g[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = i; j < 8; ++j) {
                const double s = wsum(in ? ju[i] * ju[j] + jv[i] * jv[j] : 0.0);
                A[i][j] = s; A[j][i] = s;
            }
            g[i] = -wsum(in ? ju[i] * eu + jv[i] * ev : 0.0);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) A[i][i] += lam * A[i][i];
        double step[8], hn[8];
        double c1 = INFINITY;
        if (chol_solve<8>(A, g, step)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) hn[i] = h[i] + step[i];
            c1 = cost(hn);
        }
        if (c1 < c0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) h[i] = hn[i];
            c0 = c1;
            lam = fmax(lam * 0.1, 1e-12);
        } else {
            lam *= 10.0;
        }
    }
    // H = Td^-1 * Hn * Ts
    const double Hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
    const double Ts[9] = {ss, 0, -ss * csx, 0, ss, -ss * csy, 0, 0, 1};
    const double Ti[9] = {1 / sd, 0, cdx, 0, 1 / sd, cdy, 0, 0, 1};
    double t1[9];
    mul33(Hn, Ts, t1);
    mul33(Ti, t1, H);
    if (fabs(H[8]) < 1e-300) return false;
    const double s8 = H[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] /= s8;
    return true;
}

// cv2.findHomography(src, dst, RANSAC, thr) restated (ellipse.py:496-498)
__device__ bool homography_ransac(u64 mask, double sx, double sy, double du, double dv, double thr, double* H) {
    const int lane = threadIdx.x & 63;
    const int n = popc64(mask);
    if (n < 4) return false;
    Best mine{-1, INFINITY, 1 << 30};
    double Hm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int round = 0; round < 2; ++round) {
        const int h = round * 64 + lane;
        int idx[4] = {0, 0, 0, 0};
        bool ok = sample4(h, n, idx);
        double s[4][2], d[4][2];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int src = kth_set_bit(mask, idx[k]);
            s[k][0] = __shfl(sx, src, 64); s[k][1] = __shfl(sy, src, 64);
            d[k][0] = __shfl(du, src, 64); d[k][1] = __shfl(dv, src, 64);
        }
        double Hh[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // never read uninitialised (a failed hypothesis keeps zeros)
        ok = ok && homography_4pt(s, d, Hh);
        int cnt = 0;
        double se = 0;
        for (u64 m = mask; m; m &= m - 1) {
            const int j = __ffsll((long long)m) - 1;
            const double x = bcast(sx, j), y = bcast(sy, j), u = bcast(du, j), v = bcast(dv, j);
            if (ok) {
                double pu, pv;
                apply_h(Hh, x, y, pu, pv);
                const double e2 = (pu - u) * (pu - u) + (pv - v) * (pv - v);
                if (e2 <= thr * thr) { ++cnt; se += e2; }
            }
        }
        const Best cand{ok ? cnt : -1, ok ? se : INFINITY, h};
        const bool take = ok && better(cand, mine);
        mine.cnt = take ? cand.cnt : mine.cnt; mine.s = take ? cand.s : mine.s; mine.h = take ? cand.h : mine.h;
#pragma unroll
        for (int i = 0; i < 9; ++i) Hm[i] = take ? Hh[i] : Hm[i];
    }
    const Best best = wave_best(mine);
    if (best.cnt < 4) return false;
    const int owner = best.h & 63;
    double Hb[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Hb[i] = bcast(Hm[i], owner);
    double pu, pv;
    apply_h(Hb, sx, sy, pu, pv);
    const double e2 = (pu - du) * (pu - du) + (pv - dv) * (pv - dv);
    const u64 inl = __ballot(((mask >> lane) & 1) && e2 <= thr * thr);
    return homography_lsq(inl, sx, sy, du, dv, 10, H);
}

// camera.py:366-426 in closed form: w = (a,0,a,b,(cy/cx)b,c) spans the null space of the 5x6 system
__device__ bool k_from_homography(const double* H, double cx, double cy, double& fx, double& fy) {
    const double k = cy / cx;
    const double r3[3] = {H[0] * H[1] + H[3] * H[4], (H[0] * H[7] + H[1] * H[6]) + k * (H[3] * H[7] + H[4] * H[6]), H[6] * H[7]};
    const double r4[3] = {(H[0] * H[0] - H[1] * H[1]) + (H[3] * H[3] - H[4] * H[4]),
                          (2 * H[0] * H[6] - 2 * H[1] * H[7]) + k * (2 * H[3] * H[6] - 2 * H[4] * H[7]),
                          H[6] * H[6] - H[7] * H[7]};
    const double a = r3[1] * r4[2] - r3[2] * r4[1], b = r3[2] * r4[0] - r3[0] * r4[2], c = r3[0] * r4[1] - r3[1] * r4[0];
    if (c == 0) return false;
    const double W00 = a / c, W02 = b / c, W12 = k * b / c;
    if (!(W00 > 0)) return false;
    const double L00 = sqrt(W00), L20 = W02 / L00, L21 = W12 / L00;   // W11 == W00
    const double d = 1.0 - L20 * L20 - L21 * L21;
    if (!(d > 0)) return false;
    const double L22 = sqrt(d);
    fx = L22 / L00; fy = L22 / L00;
    return true;
}

}  // namespace
