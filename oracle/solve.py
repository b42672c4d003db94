"""Oracle: CPU restatement (numpy fp64) of the camera solve.  TEST INFRASTRUCTURE ONLY.

*** PARITY UNPINNED ***  The arithmetic of this stage lives in opencv-python==4.7.0.72
(/root/reference/requirements.txt:5: cv2.calibrateCamera, cv2.findHomography, cv.solvePnPRansac,
cv.solvePnPRefineLM, cv2.Rodrigues), which is neither vendored in /root/reference nor installable
offline, and the reference holds no test / golden vector for it.  The CONTROL FLOW below follows the
reference line by line; the numerical routines are the build's own restatement of the published
algorithms, and are pinned only by (1) synthetic known-camera recovery, (2) an independent
scipy.optimize.least_squares cross-check of every minimiser, (3) fixtures under tests/golden/.

Control flow followed (file:line under /root/reference/src/models/hrnet/prediction.py):
  CameraCreator.__call__ :130-136      iterative_voter :245-257     voter :259-330
  original_voter :339-437              get_camera_from_homography :487-520
  get_camera_all_points :523-555 (view duplication quirk Q1, always-PnP quirk Q2)
  _reliable_points :558-562   _groundplane_points :565-569   _accurate_points :572-606
  get_camera_gen :609-640     good_camera / is_good_camera :469-484
  opencv_calibration :138-170          opencv_calibration_multiplane :172-243
and baseline/camera.py: solve_pnp :92-103, refine_camera :105-119, projection_rmse :270-277,
estimate_calibration_matrix_from_plane_homography :366-426; src/datatools/ellipse.py:496-498.

Numerical routines (shared specification with csrc/solve.hip, which implements them independently):
  homography_ransac   4-point hypotheses (closed-form projective-basis map) drawn by a counter-based
                      hash, inliers at thr px, refit = normalised least squares + damped Gauss-Newton
                      on the reprojection error              (restates cv2.findHomography(RANSAC))
  k_from_homography   IAC constraints of camera.py:366-426 solved in closed form
  pose_from_homography / pnp_ransac   planar minimal solver on ground points, 8 px inliers, LM refit
                      (restates cv.solvePnPRansac defaults: 8 px, SOLVEPNP_ITERATIVE refit)
  refine_pose_lm      Levenberg-Marquardt on the 6-DoF pose, K fixed, run to convergence
                      (restates cv.solvePnPRefineLM with criteria (20000, 1e-5))
  calibrate_planes    Zhang initialisation (vanishing-point focal estimate, pp=((w-1)/2,(h-1)/2),
                      aspect 1) + joint LM over {f, per-view pose}, distortion fixed to zero
                      (restates cv2.calibrateCamera with the flags of prediction.py:398-404)
Because every minimiser is run to convergence, the result is the minimum itself and does not depend on
OpenCV's iteration trajectory; where OpenCV stops early (<=30 joint iterations) results may differ.
"""
from __future__ import annotations

import numpy as np

from . import camera_math as cm
from .pitch import GOAL_LEFT, GOAL_RIGHT, GROUND, KEEP_POINTS, TOP_GATES, pitch_points

# Stopping rules of the minimisers and the handling of a failed IAC factorisation (shared with csrc/solve.hip).  Default since round
# 3 / 4: OpenCV's schedules as far as they are known (`opencv_stops()`: calibrateCamera's default criteria of 30 joint iterations,
# solvePnPRefineLM's criteria (20000, 1e-5) on step and residual; SURVEY 8c notes) and `iac_failure='reference'` = go on with
# K = I as prediction.py:514 does.  tools/solve_schedule_sweep.py switches them (`converged_stops()`, `iac_failure='drop'` = rounds
# 1-3: the homography camera is unavailable) to bound the UNPINNED gap to OpenCV.
STOP = dict(schedule='opencv', joint_iters=30, pose_iters=20000, pose_eps=1e-5, pose_res_eps=1e-5, iac_failure='reference')
COUNTERS = dict(iac_failures=0, refine_cap_hits=0)
FLT_EPSILON = 1.1920928955078125e-07
DBL_EPSILON = 2.220446049250313e-16


def opencv_stops(pose_iters=20000):
    """pose_iters: cap of refine_camera's LMSolver run = the reference's 20000 (camera.py:116; shared with solve.hip,
    sncal_voter_cfg.refine_max_iters; rounds 1-3 capped it at 200).  Well-posed frames stop on the 1e-5 step test within ~25
    iterations; the runs that used to reach the cap were poses refined under a degenerate calibration (f ~ 0.04 px candidates of the
    voter: LMSolver crawls through reject / accept / accept rounds that gain 1e-4 of the error each) -- those candidates are no longer
    refined at all (camera_all_points: their focal length fails good_camera whatever the pose), the few that remain are slow fits
    of real cameras, which the reference runs to the end as well.
    DEFAULT since round 3: the minimisers follow OpenCV 4.7's own schedules as far as they are known (SURVEY 8c notes, restated
    from the upstream sources from memory -- still UNPINNED): LMSolver for solvePnPRefineLM (lm_solver_pose), CvLevMarq for the
    extrinsics refinements (cvlevmarq_pose, 20 iterations / FLT_EPSILON) and for calibrateCamera's joint fit (30 / DBL_EPSILON)."""
    STOP.update(schedule='opencv', joint_iters=30, pose_iters=pose_iters, pose_eps=1e-5, pose_res_eps=1e-5)


def converged_stops():
    """The build's round-1/2 specification: every minimiser runs to convergence under its own x10 / /10 damping schedule."""
    STOP.update(schedule='converged', joint_iters=60, pose_iters=100, pose_eps=1e-10, pose_res_eps=0.0)


P64 = pitch_points()
P32 = P64.astype(np.float32).astype(np.float64)     # what cv2 sees: np.array(..., dtype=np.float32)
PLANES = (('groundplane', GROUND, False), ('goal_left', GOAL_LEFT, True), ('goal_right', GOAL_RIGHT, True))
NH_HOMOGRAPHY = 128
NH_PNP = 64
MASK64 = (1 << 64) - 1


def _mix(h: int, j: int) -> int:
    """splitmix64-style counter hash: the shared RANSAC sampler (hypothesis h, draw j)."""
    z = (h * 0x9E3779B97F4A7C15 + j * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return (z ^ (z >> 31)) & MASK64


def sample4(h: int, n: int):
    """4 distinct indices in [0,n) for hypothesis h, or None (shared spec with solve.hip)."""
    out = []
    for j in range(16):
        idx = int((_mix(h, j) >> 32) % n)
        if idx not in out:
            out.append(idx)
            if len(out) == 4:
                return out
    return None


def chol_solve(A, b, rel_tol=1e-11):
    """Solve the SPD system A x = b by Cholesky; None when a pivot falls below rel_tol * max diag
    (rank-deficient normal equations: collinear points, under-determined views).  Shared spec."""
    n = len(b)
    L = np.zeros((n, n))
    dmax = float(np.max(np.diag(A)))
    if not dmax > 0:
        return None
    for j in range(n):
        d = A[j, j] - float(L[j, :j] @ L[j, :j])
        if not d > rel_tol * dmax:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - float(L[i, :j] @ L[j, :j])) / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - float(L[i, :i] @ y[:i])) / L[i, i]
    x = np.zeros(n)
    for i in reversed(range(n)):
        x[i] = (y[i] - float(L[i + 1:, i] @ x[i + 1:])) / L[i, i]
    return x


# ------------------------------------------------------------------------------------------------
# homography
# ------------------------------------------------------------------------------------------------

def _basis_map(p):
    """3x3 map sending the canonical projective basis to the 4 points p (4,2); None if degenerate."""
    M = np.array([[p[0, 0], p[1, 0], p[2, 0]], [p[0, 1], p[1, 1], p[2, 1]], [1.0, 1.0, 1.0]])
    det = np.linalg.det(M)
    scale = max(1.0, np.abs(p).max()) ** 2
    if abs(det) < 1e-9 * scale:
        return None
    lam = np.linalg.solve(M, np.array([p[3, 0], p[3, 1], 1.0]))
    if np.min(np.abs(lam)) < 1e-9:
        return None
    return M * lam[None, :]


def homography_4pt(src, dst):
    A = _basis_map(src)
    B = _basis_map(dst)
    if A is None or B is None:
        return None
    detA = np.linalg.det(A)
    if abs(detA) < 1e-300:
        return None
    H = B @ np.linalg.inv(A)
    if abs(H[2, 2]) < 1e-12:
        return None
    return H / H[2, 2]


def _apply_h(H, xy):
    q = np.c_[xy, np.ones(len(xy))] @ H.T
    w = np.where(np.abs(q[:, 2]) < 1e-300, 1e-300, q[:, 2])
    return q[:, :2] / w[:, None]


def homography_lsq(src, dst, iters: int = 10):
    """Normalised inhomogeneous least squares (h33 = 1) + damped Gauss-Newton on reprojection error."""
    n = len(src)
    cs, cd = src.mean(0), dst.mean(0)
    ss = np.sqrt(2.0) / max(np.mean(np.linalg.norm(src - cs, axis=1)), 1e-12)
    sd = np.sqrt(2.0) / max(np.mean(np.linalg.norm(dst - cd, axis=1)), 1e-12)
    x, y = ((src - cs) * ss).T
    u, v = ((dst - cd) * sd).T
    A = np.zeros((2 * n, 8))
    b = np.zeros(2 * n)
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = x, y, 1
    A[0::2, 6], A[0::2, 7] = -u * x, -u * y
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = x, y, 1
    A[1::2, 6], A[1::2, 7] = -v * x, -v * y
    b[0::2], b[1::2] = u, v
    h = chol_solve(A.T @ A, A.T @ b)
    if h is None:
        return None
    lam = 1e-3
    def cost(hh):
        Hn = np.append(hh, 1.0).reshape(3, 3)
        r = _apply_h(Hn, np.c_[x, y]) - np.c_[u, v]
        return float((r ** 2).sum())
    c0 = cost(h)
    for _ in range(iters):
        Hn = np.append(h, 1.0).reshape(3, 3)
        q = np.c_[x, y, np.ones(n)] @ Hn.T
        w = q[:, 2]
        pu, pv = q[:, 0] / w, q[:, 1] / w
        J = np.zeros((2 * n, 8))
        J[0::2, 0], J[0::2, 1], J[0::2, 2] = x / w, y / w, 1 / w
        J[0::2, 6], J[0::2, 7] = -pu * x / w, -pu * y / w
        J[1::2, 3], J[1::2, 4], J[1::2, 5] = x / w, y / w, 1 / w
        J[1::2, 6], J[1::2, 7] = -pv * x / w, -pv * y / w
        r = np.zeros(2 * n)
        r[0::2], r[1::2] = pu - u, pv - v
        JTJ, g = J.T @ J, J.T @ r
        step = chol_solve(JTJ + lam * np.diag(np.diag(JTJ)), -g)
        c1 = cost(h + step) if step is not None else np.inf
        if c1 < c0:
            h, c0, lam = h + step, c1, max(lam * 0.1, 1e-12)
        else:
            lam *= 10.0
    Hn = np.append(h, 1.0).reshape(3, 3)
    Ts = np.array([[ss, 0, -ss * cs[0]], [0, ss, -ss * cs[1]], [0, 0, 1]])
    Td_inv = np.array([[1 / sd, 0, cd[0]], [0, 1 / sd, cd[1]], [0, 0, 1]])
    H = Td_inv @ Hn @ Ts
    if abs(H[2, 2]) < 1e-300:
        return None
    return H / H[2, 2]


def homography_ransac(src, dst, thr: float):
    """ellipse.py:496-498 get_homography(world, img, thr) = cv2.findHomography(.., cv2.RANSAC, thr)[0]."""
    n = len(src)
    if n < 4:
        return None
    best = (-1, np.inf, -1, None)
    for h in range(NH_HOMOGRAPHY):
        idx = sample4(h, n)
        if idx is None:
            continue
        H = homography_4pt(src[idx], dst[idx])
        if H is None:
            continue
        e2 = ((_apply_h(H, src) - dst) ** 2).sum(1)
        inl = e2 <= thr * thr
        cnt, s = int(inl.sum()), float(e2[inl].sum())
        if cnt > best[0] or (cnt == best[0] and s < best[1]):
            best = (cnt, s, h, inl)
    if best[0] < 4:
        return None
    inl = best[3]
    return homography_lsq(src[inl], dst[inl])


# ------------------------------------------------------------------------------------------------
# pose
# ------------------------------------------------------------------------------------------------

def _polar(R):
    """Nearest rotation (Newton iteration of the polar decomposition; det>0 enforced)."""
    if np.linalg.det(R) < 0:
        R = R.copy()
        R[:, 2] *= -1
    for _ in range(12):
        R = 0.5 * (R + np.linalg.inv(R).T)
    return R


def exp_so3(w):
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def pose_from_homography(H, fx, fy, cx, cy):
    """camera.py:136-153 (H = K [r1 r2 t] for the z=0 plane).  Returns (R, t) or None."""
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])
    hp = Kinv @ H
    n0, n1 = np.linalg.norm(hp[:, 0]), np.linalg.norm(hp[:, 1])
    if n0 < 1e-300 or n1 < 1e-300:
        return None
    l1, l2 = 1 / n0, 1 / n1
    r0, r1 = hp[:, 0] * l1, hp[:, 1] * l2
    t = hp[:, 2] * np.sqrt(l1 * l2)
    if t[2] < 0:          # plane must be in front of the camera
        r0, r1, t = -r0, -r1, -t
    R = _polar(np.column_stack([r0, r1, np.cross(r0, r1)]))
    return R, t


def project(R, t, K4, X):
    """Pinhole projection with K4 = (fx, fy, cx, cy); returns (N,2) and z."""
    Xc = X @ R.T + t
    z = Xc[:, 2]
    zs = np.where(np.abs(z) < 1e-12, 1e-12, z)
    return np.c_[K4[0] * Xc[:, 0] / zs + K4[2], K4[1] * Xc[:, 1] / zs + K4[3]], z


def refine_pose_lm(R, t, K4, X, uv, max_iters: int = 100, eps: float = 1e-10):
    """camera.py:105-119 refine_camera: LM over the 6-DoF pose (left perturbation R<-exp(w)R), K fixed."""
    def cost(R_, t_):
        p, _ = project(R_, t_, K4, X)
        return float(((p - uv) ** 2).sum())
    lam = 1e-3
    c0 = cost(R, t)
    for _ in range(max_iters):
        Xc = X @ R.T + t
        z = np.where(np.abs(Xc[:, 2]) < 1e-12, 1e-12, Xc[:, 2])
        x, y = Xc[:, 0] / z, Xc[:, 1] / z
        r = np.zeros(2 * len(X))
        r[0::2], r[1::2] = K4[0] * x + K4[2] - uv[:, 0], K4[1] * y + K4[3] - uv[:, 1]
        J = np.zeros((2 * len(X), 6))
        # d(u)/d(Xc) = fx*[1/z, 0, -x/z];  dXc/dw = -[Xc]x ; dXc/dt = I
        du = np.c_[K4[0] / z, np.zeros_like(z), -K4[0] * x / z]
        dv = np.c_[np.zeros_like(z), K4[1] / z, -K4[1] * y / z]
        for row, d in ((0, du), (1, dv)):
            J[row::2, 0] = d[:, 2] * Xc[:, 1] - d[:, 1] * Xc[:, 2]     # (d x Xc... ) = d . (-[Xc]x e_k)
            J[row::2, 1] = d[:, 0] * Xc[:, 2] - d[:, 2] * Xc[:, 0]
            J[row::2, 2] = d[:, 1] * Xc[:, 0] - d[:, 0] * Xc[:, 1]
            J[row::2, 3:6] = d
        A, g = J.T @ J, J.T @ r
        if STOP['pose_res_eps'] > 0 and np.abs(r).max() < STOP['pose_res_eps']:
            break
        improved = False
        for _try in range(12):
            step = chol_solve(A + np.diag(np.diag(A)) * lam, -g)
            if step is None:
                lam *= 10
                continue
            Rn, tn = exp_so3(step[:3]) @ R, exp_so3(step[:3]) @ t + step[3:]
            c1 = cost(Rn, tn)
            if c1 < c0:
                R, t, lam, improved = Rn, tn, max(lam * 0.1, 1e-15), True
                dc, c0 = c0 - c1, c1
                break
            lam *= 10
        if not improved or np.abs(step).max() < eps or dc <= 1e-16 * max(c0, 1e-30):
            break
    return _polar(R), t


# ------------------------------------------------------------------------------------------------
# OpenCV's own minimiser schedules (opencv-python 4.7.0.72, restated from the upstream sources from memory: UNPINNED)
# ------------------------------------------------------------------------------------------------

def log_so3(R):
    """cv.Rodrigues(matrix -> vector) for an orthonormal R: axis * angle."""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) * 0.5))
    th = np.arccos(c)
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * 0.5          # sin(th) * axis
    s = np.linalg.norm(a)
    if s < 1e-5:
        if c > 0:
            return a.copy()                                   # th ~ 0: r ~ the antisymmetric part
        # th ~ pi: axis from the symmetric part (R + I) / 2 = axis axis^T, sign from the antisymmetric part where it still speaks
        B = (R + np.eye(3)) * 0.5
        ax = np.sqrt(np.maximum(np.diag(B), 0.0))
        k = int(np.argmax(ax))
        ax = B[:, k] / max(ax[k], 1e-300)
        ax = ax / max(np.linalg.norm(ax), 1e-300)
        if a @ ax < 0:
            ax = -ax
        return ax * th
    return a * (th / s)


def left_jacobian_so3(r):
    """exp(r + d) ~ exp(J_l(r) d) exp(r): J_l = I + (1 - cos th)/th^2 [r]x + (th - sin th)/th^3 [r]x^2."""
    th = np.linalg.norm(r)
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    if th < 1e-6:
        return np.eye(3) + 0.5 * K + K @ K / 6.0
    return np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * (K @ K)


def pose_rows_rvec(rvec, tvec, K4, X, uv):
    """cv.projectPoints' residual (projected - observed, x/y interleaved) and Jacobian wrt (rvec, tvec), Rodrigues
    parameterisation (analytically equal to OpenCV's dpdr / dpdt); also the normalised coordinates (the focal column)."""
    R = exp_so3(rvec)
    Xr = X @ R.T
    Xc = Xr + tvec
    z = np.where(np.abs(Xc[:, 2]) < 1e-12, 1e-12, Xc[:, 2])
    x, y = Xc[:, 0] / z, Xc[:, 1] / z
    n = len(X)
    r = np.zeros(2 * n)
    r[0::2], r[1::2] = K4[0] * x + K4[2] - uv[:, 0], K4[1] * y + K4[3] - uv[:, 1]
    du = np.c_[K4[0] / z, np.zeros(n), -K4[0] * x / z]
    dv = np.c_[np.zeros(n), K4[1] / z, -K4[1] * y / z]
    Jl = left_jacobian_so3(rvec)
    J = np.zeros((2 * n, 6))
    for row, d in ((0, du), (1, dv)):
        # d . (w x Xr) = w . (Xr x d): rotation about the camera origin moves the ROTATED point only (tvec is its own parameter)
        wrow = np.cross(Xr, d)
        J[row::2, 0:3] = wrow @ Jl
        J[row::2, 3:6] = d
    jf = np.zeros(2 * n)
    jf[0::2], jf[1::2] = x, y
    return r, J, jf


def sym_solve(A, b):
    """cv::solve(A, b, DECOMP_EIG / DECOMP_SVD) for a symmetric system: Cholesky when A is positive definite, else the
    minimum-norm solution with eigenvalues below 2 eps trace(|w|) dropped (shared spec with solve.hip)."""
    x = chol_solve(A, b)
    if x is not None:
        return x
    w, V = np.linalg.eigh(A)
    thr = 2.0 * DBL_EPSILON * np.abs(w).sum()
    inv = np.where(np.abs(w) > thr, 1.0 / np.where(w == 0, 1.0, w), 0.0)
    return V @ (inv * (V.T @ b))


def lm_solver_pose(R, t, K4, X, uv, max_iters=20000, eps=1e-5):
    """cv.solvePnPRefineLM = LMSolver::run (calib3d levmarq.cpp) on x = [rvec, tvec]: D = diag(J^T J) FIXED at the start,
    lambda_0 = 1, step d solves (A + lambda D) d = J^T r, x' = x - d, gain ratio R = (S - S') / d.(2 v - A d):
    R > 0.75 -> lambda /= 2 (to 0 below lambda_c = 0.75); R < 0.25 -> lambda *= nu, nu = clip((S' - S) / (d.v) + 2, 2, 10)
    (from lambda = 0: lambda = lambda_c = 1 / max |diag(A^-1)|, nu /= 2); accept when S' < S; stop after max_iters, or when
    |d|_inf < eps, or |r|_inf < eps.  camera.py:105-119 passes (20000, 1e-5)."""
    x = np.r_[log_so3(R), t].astype(np.float64)
    r, J, _ = pose_rows_rvec(x[:3], x[3:], K4, X, uv)
    S = float(r @ r)
    A, v = J.T @ J, J.T @ r
    D = np.diag(A).copy()
    lam, lc = 1.0, 0.75
    it = 0
    while True:
        d = sym_solve(A + np.diag(lam * D), v)
        xd = x - d
        rd, Jd, _ = pose_rows_rvec(xd[:3], xd[3:], K4, X, uv)
        Sd = float(rd @ rd)
        dS = float(d @ (2.0 * v - A @ d))
        Rg = (S - Sd) / (dS if abs(dS) > DBL_EPSILON else 1.0)
        if Rg > 0.75:
            lam *= 0.5
            if lam < lc:
                lam = 0.0
        elif Rg < 0.25:
            tq = float(d @ v)
            nu = (Sd - S) / (tq if abs(tq) > DBL_EPSILON else 1.0) + 2.0
            nu = min(max(nu, 2.0), 10.0)
            if lam == 0.0:
                Ainv = np.column_stack([sym_solve(A, e) for e in np.eye(6)])
                lam = lc = 1.0 / max(DBL_EPSILON, float(np.abs(np.diag(Ainv)).max()))
                nu *= 0.5
            lam *= nu
        if Sd < S:
            S, x, r, J = Sd, xd, rd, Jd
            A, v = J.T @ J, J.T @ r
        it += 1
        if not (it < max_iters and np.abs(d).max() >= eps and np.abs(r).max() >= eps):
            break
    COUNTERS['refine_iters_max'] = max(COUNTERS.get('refine_iters_max', 0), it)
    if it >= max_iters:
        COUNTERS['refine_cap_hits'] += 1
    return exp_so3(x[:3]), x[3:].copy()


def _cvlevmarq(evaluate, solve_step, x0, max_iter, eps):
    """CvLevMarq::update / updateAlt (calib3d compat_ptsetreg.cpp): lambda = 10^k, k_0 = -3; a step solves
    (J^T J with its diagonal x (1 + lambda)) d = J^T r from the SAME normal equations until the error no longer grows
    (k += 1 per rejection, up to 16; then the step is taken regardless); an accepted step lowers k by one and counts as an
    iteration; stop after max_iter iterations or when |x - x_prev| / |x_prev| < eps.
    evaluate(x) -> (err, normal equations or None); solve_step(normal equations, lambda) -> d or None."""
    x = x0
    k = -3
    e_prev, ne = evaluate(x, True)
    iters = 0
    while True:
        prev = x
        d = solve_step(ne, 10.0 ** k)
        cand = prev - d if d is not None else None
        e = evaluate(cand, False)[0] if cand is not None else np.inf
        while e > e_prev:
            k += 1
            if k > 16:
                break
            d = solve_step(ne, 10.0 ** k)
            cand = prev - d if d is not None else None
            e = evaluate(cand, False)[0] if cand is not None else np.inf
        if cand is None or not np.isfinite(e):
            return prev                         # no usable step at any damping (singular normal equations): keep the last parameters
        k = max(k - 1, -16)
        x = cand
        iters += 1
        if iters >= max_iter or np.linalg.norm(x - prev) / max(np.linalg.norm(prev), 1e-300) < eps:
            return x
        e_prev, ne = evaluate(x, True)


def cvlevmarq_pose(R, t, K4, X, uv, max_iter=20, eps=FLT_EPSILON):
    """cvFindExtrinsicCameraParams2's refinement (the SOLVEPNP_ITERATIVE refit of solvePnPRansac and the per-view initial
    extrinsics of calibrateCamera): CvLevMarq over [rvec, tvec], criteria (20, FLT_EPSILON)."""
    def evaluate(x, want_j):
        r, J, _ = pose_rows_rvec(x[:3], x[3:], K4, X, uv)
        return float(r @ r), ((J.T @ J, J.T @ r) if want_j else None)

    def solve_step(ne, lam):
        A, g = ne
        return sym_solve(A + lam * np.diag(np.diag(A)), g)        # cv::solve(..., DECOMP_SVD): a step even when not positive definite
    x = _cvlevmarq(evaluate, solve_step, np.r_[log_so3(R), t].astype(np.float64), max_iter, eps)
    return exp_so3(x[:3]), x[3:].copy()


def _joint_cvlevmarq(views, weights, f, poses, cx, cy, max_iter, eps):
    """calibrateCamera's joint fit (cvCalibrateCamera2Internal) under the reference's flags (prediction.py:398-404, 614-620):
    free parameters fy (fx slaved, aspect 1) and [rvec, tvec] per view; identical duplicated views (Q1) collapse to weights.
    Block-arrowhead normal equations solved through the Schur complement on f (equal to OpenCV's dense SVD solve whenever the
    pose blocks are non-singular)."""
    nv = len(views)
    x0 = np.r_[f, np.concatenate([np.r_[log_so3(R_), t_] for R_, t_ in poses])]

    def evaluate(x, want_j):
        if not x[0] > 0:
            return np.inf, None
        err, blocks, aff, gf = 0.0, [], 0.0, 0.0
        for vi, ((Xp, uv), wgt) in enumerate(zip(views, weights)):
            p = x[1 + 6 * vi: 7 + 6 * vi]
            r, J, jf = pose_rows_rvec(p[:3], p[3:], (x[0], x[0], cx, cy), Xp, uv)
            err += wgt * float(r @ r)
            if want_j:
                blocks.append((wgt * J.T @ J, wgt * J.T @ jf, wgt * J.T @ r))
                aff += wgt * float(jf @ jf)
                gf += wgt * float(jf @ r)
        return err, ((blocks, aff, gf) if want_j else None)

    def solve_step(ne, lam):
        blocks, aff, gf = ne
        s_aff, s_g, sol = aff * (1 + lam), gf, []
        for A_, B_, g_ in blocks:
            Ad = A_ + lam * np.diag(np.diag(A_))
            ab, ag = sym_solve(Ad, B_), sym_solve(Ad, g_)      # (OpenCV: one dense SVD solve; the pose blocks never abort the step)
            s_aff -= float(B_ @ ab)
            s_g -= float(B_ @ ag)
            sol.append((ab, ag))
        if abs(s_aff) < 1e-300:
            return None
        df = s_g / s_aff
        return np.r_[df, np.concatenate([ag - ab * df for ab, ag in sol])]
    x = _cvlevmarq(evaluate, solve_step, x0, max_iter, eps)
    return float(x[0]), [[exp_so3(x[1 + 6 * vi: 4 + 6 * vi]), x[4 + 6 * vi: 7 + 6 * vi].copy()] for vi in range(nv)]


def polish4(R, t, K4, X4, uv4):
    """Damped Gauss-Newton polish of a minimal-sample pose on its own 4 points (shared spec with solve.hip):
    the closed-form homography decomposition is badly conditioned for long focal lengths."""
    def cost(R_, t_):
        p, _ = project(R_, t_, K4, X4)
        return float(((p - uv4) ** 2).sum())
    c0 = cost(R, t)
    for _ in range(8):
        Xc = X4 @ R.T + t
        z = np.where(np.abs(Xc[:, 2]) < 1e-12, 1e-12, Xc[:, 2])
        x, y = Xc[:, 0] / z, Xc[:, 1] / z
        r = np.zeros(8)
        r[0::2], r[1::2] = K4[0] * x + K4[2] - uv4[:, 0], K4[1] * y + K4[3] - uv4[:, 1]
        J = np.zeros((8, 6))
        du = np.c_[K4[0] / z, np.zeros_like(z), -K4[0] * x / z]
        dv = np.c_[np.zeros_like(z), K4[1] / z, -K4[1] * y / z]
        for row, d in ((0, du), (1, dv)):
            J[row::2, 0] = d[:, 2] * Xc[:, 1] - d[:, 1] * Xc[:, 2]
            J[row::2, 1] = d[:, 0] * Xc[:, 2] - d[:, 2] * Xc[:, 0]
            J[row::2, 2] = d[:, 1] * Xc[:, 0] - d[:, 0] * Xc[:, 1]
            J[row::2, 3:6] = d
        A = J.T @ J
        step = chol_solve(A + 1e-3 * np.diag(np.diag(A)), -(J.T @ r))
        if step is None:
            break
        E = exp_so3(step[:3])
        Rn, tn = E @ R, E @ t + step[3:]
        c1 = cost(Rn, tn)
        if not c1 < c0:
            break
        R, t, c0 = Rn, tn, c1
    return R, t


def pnp_ransac(K4, X, uv, ground_mask):
    """camera.py:92-103 solve_pnp = cv.solvePnPRansac(obj, img, K, None) + Rodrigues.
    Minimal solver: planar pose from 4 ground points; inliers at 8 px; LM refit on the inliers.
    Returns (R, t) or None."""
    gi = np.nonzero(ground_mask)[0]
    n = len(gi)
    best = (-1, np.inf, None)
    if n >= 4:
        for h in range(NH_PNP):
            idx = sample4(h, n)
            if idx is None:
                continue
            sel = gi[idx]
            H = homography_4pt(X[sel, :2], uv[sel])
            if H is None:
                continue
            pose = pose_from_homography(H, *K4)
            if pose is None:
                continue
            X4 = np.c_[X[sel, :2], np.zeros(4)]
            pose = polish4(pose[0], pose[1], K4, X4, uv[sel])
            p, z = project(pose[0], pose[1], K4, X)
            e2 = ((p - uv) ** 2).sum(1)
            inl = (e2 <= 64.0) & (z > 1e-9)
            cnt, s = int(inl.sum()), float(e2[inl].sum())
            if cnt > best[0] or (cnt == best[0] and s < best[1]):
                best = (cnt, s, (pose, inl))
    if n >= 4:      # hypothesis NH_PNP: least-squares homography over every z=0 point
        H = homography_lsq(X[gi, :2], uv[gi], iters=10)
        pose = pose_from_homography(H, *K4) if H is not None else None
        if pose is not None:
            pose = _refit(pose[0], pose[1], K4, X[gi], uv[gi])
            p, z = project(pose[0], pose[1], K4, X)
            e2 = ((p - uv) ** 2).sum(1)
            inl = (e2 <= 64.0) & (z > 1e-9)
            cnt, s = int(inl.sum()), float(e2[inl].sum())
            if cnt > best[0] or (cnt == best[0] and s < best[1]):
                best = (cnt, s, (pose, inl))
    if best[0] < 4:
        return None
    (R, t), inl = best[2]
    return _refit(R, t, K4, X[inl], uv[inl])


def _refit(R, t, K4, X, uv):
    """The 20-iteration pose refinement inside solvePnPRansac's final SOLVEPNP_ITERATIVE call and calibrateCamera's per-view
    initial extrinsics (cvFindExtrinsicCameraParams2)."""
    if STOP['schedule'] == 'opencv':
        return cvlevmarq_pose(R, t, K4, X, uv, max_iter=20, eps=FLT_EPSILON)
    return refine_pose_lm(R, t, K4, X, uv, max_iters=20)


# ------------------------------------------------------------------------------------------------
# calibrateCamera restatement
# ------------------------------------------------------------------------------------------------

def _homography_plain(src, dst):
    return homography_lsq(src, dst, iters=10)


def calibrate_planes(views, weights, img_wh):
    """views: list of (Xplane (n,3) with z=0, uv (n,2)); weights: multiplicity of each view (Q1).
    Returns (f, cx, cy, R0, t0) -- pose of views[0] -- or None."""
    cx, cy = (img_wh[0] - 1) * 0.5, (img_wh[1] - 1) * 0.5
    Hs = []
    rowsA, rowsb = [], []
    for (Xp, uv), wgt in zip(views, weights):
        H = _homography_plain(Xp[:, :2], uv)
        if H is None:
            return None
        Hs.append(H)
        Hc = H.copy()
        Hc[0] -= Hc[2] * cx
        Hc[1] -= Hc[2] * cy
        h, v = Hc[:, 0], Hc[:, 1]
        d1, d2 = (h + v) * 0.5, (h - v) * 0.5
        h, v, d1, d2 = (a / max(np.linalg.norm(a), 1e-300) for a in (h, v, d1, d2))
        sw = np.sqrt(wgt)
        rowsA += [sw * np.array([h[0] * v[0], h[1] * v[1]]), sw * np.array([d1[0] * d2[0], d1[1] * d2[1]])]
        rowsb += [-sw * h[2] * v[2], -sw * d1[2] * d2[2]]
    A, b = np.array(rowsA), np.array(rowsb)
    # 2x2 normal equations of  A [1/fx^2, 1/fy^2]^T = b  (cv's initIntrinsicParams2D solves them by SVD)
    n00, n01, n11 = float(A[:, 0] @ A[:, 0]), float(A[:, 0] @ A[:, 1]), float(A[:, 1] @ A[:, 1])
    r0, r1 = float(A[:, 0] @ b), float(A[:, 1] @ b)
    det = n00 * n11 - n01 * n01
    if not abs(det) > 1e-14 * max(n00 * n11, 1e-300):
        return None
    sol = np.array([(n11 * r0 - n01 * r1) / det, (n00 * r1 - n01 * r0) / det])
    if sol[0] == 0 or sol[1] == 0:
        return None
    fxy = np.sqrt(np.abs(1.0 / sol))
    f = float(0.5 * (fxy[0] + fxy[1]))
    if not np.isfinite(f) or f <= 0:
        return None
    poses = []
    for (Xp, uv), H in zip(views, Hs):
        pose = pose_from_homography(H, f, f, cx, cy)
        if pose is None:
            return None
        poses.append(list(_refit(pose[0], pose[1], (f, f, cx, cy), Xp, uv)))
    if STOP['schedule'] == 'opencv':
        f, poses = _joint_cvlevmarq(views, weights, f, poses, cx, cy, STOP['joint_iters'], DBL_EPSILON)
        if not np.isfinite(f) or f <= 0:
            return None
        return f, cx, cy, _polar(poses[0][0]), poses[0][1]
    # joint LM over f and the poses (block-arrowhead normal equations, Schur complement on f)
    def total_cost(f_, poses_):
        c = 0.0
        for (Xp, uv), wgt, (R_, t_) in zip(views, weights, poses_):
            p, _ = project(R_, t_, (f_, f_, cx, cy), Xp)
            c += wgt * float(((p - uv) ** 2).sum())
        return c
    lam = 1e-3
    c0 = total_cost(f, poses)
    for _ in range(STOP['joint_iters']):
        blocks = []
        aff, gf = 0.0, 0.0
        for (Xp, uv), wgt, (R_, t_) in zip(views, weights, poses):
            Xc = Xp @ R_.T + t_
            z = np.where(np.abs(Xc[:, 2]) < 1e-12, 1e-12, Xc[:, 2])
            x, y = Xc[:, 0] / z, Xc[:, 1] / z
            n = len(Xp)
            r = np.zeros(2 * n)
            r[0::2], r[1::2] = f * x + cx - uv[:, 0], f * y + cy - uv[:, 1]
            J = np.zeros((2 * n, 6))
            du = np.c_[f / z, np.zeros_like(z), -f * x / z]
            dv = np.c_[np.zeros_like(z), f / z, -f * y / z]
            for row, d in ((0, du), (1, dv)):
                J[row::2, 0] = d[:, 2] * Xc[:, 1] - d[:, 1] * Xc[:, 2]
                J[row::2, 1] = d[:, 0] * Xc[:, 2] - d[:, 2] * Xc[:, 0]
                J[row::2, 2] = d[:, 1] * Xc[:, 0] - d[:, 0] * Xc[:, 1]
                J[row::2, 3:6] = d
            jf = np.zeros(2 * n)
            jf[0::2], jf[1::2] = x, y
            blocks.append((wgt * J.T @ J, wgt * J.T @ jf, wgt * J.T @ r))
            aff += wgt * float(jf @ jf)
            gf += wgt * float(jf @ r)
        improved = False
        for _try in range(12):
            s_aff = aff * (1 + lam)
            s_g = gf
            sol_blocks = []
            ok = True
            for (A_, B_, g_) in blocks:
                Ad = A_ + lam * np.diag(np.diag(A_))
                Ainv_B = chol_solve(Ad, B_)
                Ainv_g = chol_solve(Ad, g_)
                if Ainv_B is None or Ainv_g is None:
                    ok = False
                    break
                s_aff -= float(B_ @ Ainv_B)
                s_g -= float(B_ @ Ainv_g)
                sol_blocks.append((Ainv_B, Ainv_g))
            if not ok or abs(s_aff) < 1e-300:
                lam *= 10
                continue
            df = -s_g / s_aff
            new_poses = []
            for (R_, t_), (Ainv_B, Ainv_g) in zip(poses, sol_blocks):
                step = -(Ainv_g + Ainv_B * df)
                E = exp_so3(step[:3])
                new_poses.append([E @ R_, E @ t_ + step[3:]])
            fn = f + df
            c1 = total_cost(fn, new_poses) if fn > 0 else np.inf
            if c1 < c0:
                dc = c0 - c1
                f, poses, c0, lam, improved = fn, new_poses, c1, max(lam * 0.1, 1e-15), True
                break
            lam *= 10
        if not improved or dc <= 1e-16 * max(c0, 1e-30):
            break
    return f, cx, cy, _polar(poses[0][0]), poses[0][1]


# ------------------------------------------------------------------------------------------------
# Camera record + reference control flow
# ------------------------------------------------------------------------------------------------

class Cam:
    """The attributes of baseline/camera.py:79-90 that the solve touches."""
    def __init__(self, w=960, h=540):
        self.image_width, self.image_height = w, h
        self.position = np.zeros(3)
        self.rotation = np.eye(3)
        self.calibration = np.eye(3)
        self.xfocal_length = self.yfocal_length = 1.0
        self.principal_point = (w / 2, h / 2)
        self.rmse = None
        self.tag = ''
        self.ids = None              # the point ids `rmse` is the mean over (sncal_camera.n_points = len(ids))

    @property
    def K4(self):
        K = self.calibration
        return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])

    def solve_pnp(self, ids, uv):
        ground = np.array([i not in TOP_GATES for i in ids])
        res = pnp_ransac(self.K4, P64[ids], uv, ground)
        if res is None:
            raise RuntimeError('solvePnPRansac failed')      # the reference would raise in cv.Rodrigues(None)
        R, t = res
        self.rotation, self.position = R, -R.T @ t

    def refine_camera(self, ids, uv):
        if STOP['schedule'] == 'opencv':
            R, t = lm_solver_pose(self.rotation, -self.rotation @ self.position, self.K4, P64[ids], uv,
                                  max_iters=STOP['pose_iters'], eps=STOP['pose_eps'])
        else:
            R, t = refine_pose_lm(self.rotation, -self.rotation @ self.position, self.K4, P64[ids], uv,
                                  max_iters=STOP['pose_iters'], eps=STOP['pose_eps'])
        self.rotation, self.position = R, -R.T @ t

    def projection_rmse(self, ids, uv):
        return cm.projection_rmse(self.position, self.rotation, self.xfocal_length, self.yfocal_length,
                                  self.principal_point, P64[ids], uv)


def _views_from(ids, uv32, min_pts, duplicate):
    """prediction.py:374-394 (no duplication) / :528-547 (duplication quirk Q1)."""
    views, weights, first_is_ground = [], [], None
    idset = {i: k for k, i in enumerate(ids)}
    for name, pids, swap in PLANES:
        sel = [i for i in pids if i in idset]
        if not sel:
            continue
        if duplicate:
            first = min(pids.index(i) for i in sel)
            mult = len(pids) + (1 if name == 'groundplane' else 0) - first     # range(58) holds id 57 too (Q6)
        else:
            mult = 1
        if len(sel) >= min_pts:
            X = P32[sel]
            if swap:
                X = np.c_[X[:, 1], X[:, 2], np.zeros(len(sel))]
            views.append((X, np.array([uv32[idset[i]] for i in sel])))
            weights.append(mult)
    return views, weights


def _cam_from_calibration(res, img_wh):
    f, cx, cy, R0, t0 = res
    cam = Cam(*img_wh)
    cam.calibration = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])
    cam.xfocal_length = cam.yfocal_length = f
    cam.principal_point = (img_wh[0] / 2.0, img_wh[1] / 2.0)
    cam.rotation, cam.position = R0, -R0.T @ t0
    return cam


def camera_from_homography(ids, uv, img_wh=(960, 540)):
    """prediction.py:487-520."""
    g = [k for k, i in enumerate(ids) if i in GROUND]
    if len(g) < 4:
        return None
    uv32 = uv.astype(np.float32).astype(np.float64)
    H = homography_ransac(P32[[ids[k] for k in g], :2], uv32[g], 10.0)
    if H is None:
        return None
    cam = Cam(*img_wh)
    ok, fx, fy = cm.k_from_plane_homography(H, (img_wh[0] / 2, img_wh[1] / 2))
    if not ok:
        COUNTERS['iac_failures'] += 1
        if STOP['iac_failure'] != 'reference':
            return None      # rounds 1-3 (kept for the sweeps): drop the candidate; the reference ignores the failure flag (:514) and goes on with K = I
        # the reference's path: Camera() keeps calibration = eye(3), focal lengths 1, principal point (w/2, h/2) for project_point
        cam.calibration = np.eye(3)
        cam.xfocal_length = cam.yfocal_length = 1.0
        cam.solve_pnp(ids, uv)
        cam.refine_camera(ids, uv)
        cam.ids = list(ids)
        return cam, cam.projection_rmse(ids, uv)
    cam.xfocal_length, cam.yfocal_length = fx, fy
    cam.calibration = np.array([[fx, 0, img_wh[0] / 2], [0, fy, img_wh[1] / 2], [0, 0, 1.0]])
    cam.solve_pnp(ids, uv)
    cam.refine_camera(ids, uv)
    cam.ids = list(ids)
    return cam, cam.projection_rmse(ids, uv)


def camera_all_points(ids, uv, img_wh=(960, 540)):
    """prediction.py:523-555 + get_camera_gen :609-640."""
    try:
        uv32 = uv.astype(np.float32).astype(np.float64)
        views, weights = _views_from(ids, uv32, 6, duplicate=True)
        if not (len(views) > 0 and sum(w * len(v[1]) for v, w in zip(views, weights)) > 6):
            return None
        res = calibrate_planes(views, weights, img_wh)
        if res is None:
            raise RuntimeError('calibrateCamera failed')
        cam = _cam_from_calibration(res, img_wh)
        cam.solve_pnp(ids, uv)                       # always (Q2)
        # Same outcome, less work (shared with solve.hip): every caller keeps this camera only if good_camera accepts it, and its
        # focal-length clause does not depend on the pose -- a candidate whose calibration fell outside [10, 20000] px is discarded
        # whatever refine_camera does to it, so it is not refined (under f ~ 0.04 px the reference's 20000-iteration LM runs to the end)
        if len(ids) > 6 and 10 <= cam.calibration[0, 0] <= 20000:
            cam.refine_camera(ids, uv)
        cam.ids = list(ids)
        return cam, cam.projection_rmse(ids, uv)
    except Exception:
        return None


def good_cam(cam):
    return cm.good_camera(cam.calibration[0, 0], cam.position)


class CameraCreatorOracle:
    """CameraCreator with the make_submit.py:45-50 keyword set."""

    def __init__(self, conf_thresh=0.5, conf_threshs=(0.5, 0.35, 0.2), algorithm='iterative_voter', max_rmse=55.0,
                 max_rmse_rel=5.0, min_points=5, min_focal_length=10.0, min_points_per_plane=6,
                 min_points_for_refinement=6, reliable_thresh=57, img_size=(960, 540), lines_data=None):
        self.conf_thresh, self.conf_threshs, self.algorithm = conf_thresh, conf_threshs, algorithm
        self.max_rmse, self.max_rmse_rel, self.min_points = max_rmse, max_rmse_rel, min_points
        self.min_focal_length, self.min_points_per_plane = min_focal_length, min_points_per_plane
        self.min_points_for_refinement, self.reliable_thresh = min_points_for_refinement, reliable_thresh
        self.img_size = img_size
        self.lines_data = lines_data or {}

    def __call__(self, pred, name=None):
        try:
            return getattr(self, self.algorithm)(pred, name)
        except Exception:
            return None

    def _select(self, pred, reliable_rule):
        # The reference runs on numpy 1.24 (its requirements.txt), whose value-based casting compares a float32 SCALAR with a python
        # float in double (prediction.py:181, 265, 348: float32(0.2) > 0.2 holds) but a float32 ARRAY with a python float in float32
        # (:178, 345: n_det_points does not count a confidence of exactly float32(0.2)).  Written out, so that the numpy that runs
        # this file does not decide.
        thr = float(self.conf_thresh)
        n_det = int(np.count_nonzero(pred[:, 2].astype(np.float32) > np.float32(thr)))
        ids, uv = [], []
        for i in range(pred.shape[0]):
            if float(pred[i, 2]) > thr and (not reliable_rule or n_det < self.reliable_thresh or i in KEEP_POINTS):
                ids.append(i)
                uv.append((float(pred[i, 0]), float(pred[i, 1])))
        return ids, uv

    def iterative_voter(self, pred, name):
        self.conf_thresh = 0.5
        try:
            cam = self.original_voter(pred, name)
            if cam is not None:
                return cam
        except Exception:
            pass
        for p in self.conf_threshs:
            self.conf_thresh = p
            cam = self.voter(pred, name)
            if cam is not None:
                return cam
        return None

    def original_voter(self, pred, name):
        ids, uv = self._select(pred, True)
        n_ground = sum(1 for i in ids if i not in TOP_GATES)
        for i, p in sorted(self.lines_data.get(name, {}).items()) if name is not None else []:
            if i not in ids and (n_ground < self.min_points_per_plane or
                                 (0 <= p[0] <= self.img_size[0] and 0 <= p[1] <= self.img_size[1])):
                ids.append(i)
                uv.append((float(p[0]), float(p[1])))
        uv = np.array(uv, dtype=np.float64).reshape(-1, 2)
        hom = camera_from_homography(ids, uv, self.img_size)
        cam = None
        uv32 = uv.astype(np.float32).astype(np.float64)
        views, weights = _views_from(ids, uv32, self.min_points_per_plane, duplicate=False)
        if len(views) > 0 and len(ids) > self.min_points:
            res = calibrate_planes(views, weights, self.img_size)
            if res is None:
                raise RuntimeError('calibrateCamera failed')
            cam = _cam_from_calibration(res, self.img_size)
            cam.tag = 'original'
            if sum(1 for i in ids if i in GROUND) < self.min_points_per_plane:
                cam.solve_pnp(ids, uv)
            if not good_cam(cam):
                cam = None
            elif len(ids) > self.min_points_for_refinement:
                cam.refine_camera(ids, uv)
        if cam is None and hom is not None and hom[1] < 26:
            cam = hom[0]
            cam.tag = 'original_hom'
        if cam is not None:
            cam.rmse = cam.projection_rmse(ids, uv)
            cam.ids = list(ids)
        return cam

    def voter(self, pred, name):
        ids, uv = self._select(pred, False)
        for i, p in sorted(self.lines_data.get(name, {}).items()) if name is not None else []:
            if i not in ids and sum(1 for k in ids if k in GROUND) < self.min_points_per_plane:
                ids.append(i)
                uv.append((float(p[0]), float(p[1])))
        uv = np.array(uv, dtype=np.float64).reshape(-1, 2)
        hom = camera_from_homography(ids, uv, self.img_size)

        def sub(keep):
            k = [j for j, i in enumerate(ids) if keep(i)]
            return camera_all_points([ids[j] for j in k], uv[k], self.img_size)
        c_all = camera_all_points(ids, uv, self.img_size)
        c_rel = sub(lambda i: i in KEEP_POINTS)
        c_acc = self._accurate(ids, uv, 5.0)
        c_gnd = sub(lambda i: i in GROUND)
        cams = []
        for c, tag in ((c_rel, 'camera_rel'), (c_acc, 'camera_acc'), (c_all, 'cam_all'), (c_gnd, 'cam_ground')):
            if c is not None and good_cam(c[0]):
                cams.append((c[0], c[1], tag))
        cam = None
        candidates = [(tag, r, tag == 'camera_rel' and r < self.max_rmse_rel) for _, r, tag in cams]
        if cams:
            best = max(cams, key=lambda x: (x[2] == 'camera_rel' and x[1] < self.max_rmse_rel, 1 / x[1]))
            if best[1] < self.max_rmse:
                cam = best[0]
                cam.tag, cam.rmse = best[2], best[1]
        if cam is None and hom is not None and hom[1] < self.max_rmse:
            cam = hom[0]
            cam.tag, cam.rmse = 'voter_hom', hom[1]
        if cam is not None:
            cam.candidates = candidates          # (tag, rmse, good) of the list the selection chose from
        return cam

    def _accurate(self, ids, uv, thr):
        """prediction.py:572-606."""
        g = [k for k, i in enumerate(ids) if i in GROUND]
        if len(g) < 4:
            return None
        uv32 = uv.astype(np.float32).astype(np.float64)
        W = P32[[ids[k] for k in g], :2]
        H = homography_ransac(W, uv32[g], thr)
        if H is None:
            return None
        err = np.linalg.norm(_apply_h(H, W) - uv32[g], axis=1)
        keep = [g[k] for k in range(len(g)) if err[k] < thr]
        keep += [k for k, i in enumerate(ids) if i in TOP_GATES]
        keep = sorted(set(keep), key=lambda k: (ids[k] in TOP_GATES, k))
        return camera_all_points([ids[k] for k in keep], uv[keep], self.img_size)

    def opencv_calibration(self, pred, name):
        """prediction.py:138-170: ground-plane points only, single view, pose straight from calibrateCamera."""
        ids = [i for i in range(pred.shape[0]) if i not in TOP_GATES and float(pred[i, 2]) > float(self.conf_thresh)]      # :145, a scalar
        if len(ids) <= 5:
            return None
        uv32 = pred[ids, :2].astype(np.float64)
        res = calibrate_planes([(P32[ids], uv32)], [1], self.img_size)
        if res is None:
            raise RuntimeError('calibrateCamera failed')
        cam = _cam_from_calibration(res, self.img_size)
        cam.tag = 'opencv_calibration'
        cam.rmse = cam.projection_rmse(ids, uv32)
        cam.ids = list(ids)
        return cam

    def opencv_calibration_multiplane(self, pred, name):
        """prediction.py:172-243."""
        ids, uv = self._select(pred, True)
        for i, p in sorted(self.lines_data.get(name, {}).items()) if name is not None else []:
            if i not in ids and len(ids) <= self.min_points:
                ids.append(i)
                uv.append((float(p[0]), float(p[1])))
        uv = np.array(uv, dtype=np.float64).reshape(-1, 2)
        uv32 = uv.astype(np.float32).astype(np.float64)
        views, weights = _views_from(ids, uv32, self.min_points_per_plane, duplicate=False)
        if not (len(views) > 0 and len(ids) > self.min_points):
            return None
        res = calibrate_planes(views, weights, self.img_size)
        if res is None:
            raise RuntimeError('calibrateCamera failed')
        if not res[0] > self.min_focal_length:
            return None
        cam = _cam_from_calibration(res, self.img_size)
        if len(ids) > self.min_points_for_refinement:
            cam.refine_camera(ids, uv)
        cam.tag = 'multiplane'
        cam.rmse = cam.projection_rmse(ids, uv)
        cam.ids = list(ids)
        return cam
