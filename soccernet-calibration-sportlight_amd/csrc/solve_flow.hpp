// Part of the camera solve: included by solve.hip alone (one translation unit), after solve_calib.hpp; reads solve.hip's __constant__ tables.
// The reference's control flow for the five algorithms, on the solvers of the other headers.
//
// Control flow follows the reference's CameraCreator (src/models/hrnet/prediction.py):
//   __call__ :130-136, iterative_voter :245-257, voter :259-330, original_voter :339-437,
//   get_camera_from_homography :487-520, get_camera_all_points :523-555 (+ quirks Q1/Q2),
//   _reliable/_groundplane/_accurate_points :558-606, get_camera_gen :609-640, good_camera :469-484,
//   opencv_calibration :138-170, opencv_calibration_multiplane :172-243,
// and Camera.solve_pnp / refine_camera / projection_rmse / estimate_calibration_matrix_from_plane_homography
// (baseline/camera.py:92-119, 270-277, 366-426).  The arithmetic behind the cv2 calls
// (findHomography-RANSAC, solvePnPRansac, solvePnPRefineLM, calibrateCamera) is the build's own
// restatement -- specification shared with oracle/solve.py, parity vs OpenCV itself is UNPINNED.
#pragma once

namespace {

// ---- camera record + reference control flow ----------------------------------------------------------
struct Cam {
    double R[9], pos[3];
    double fx, fy, cx, cy;      // calibration matrix (cx,cy as left by calibrateCamera: quirk Q3)
    double ppx, ppy;            // principal_point used by project_point / JSON
    double rmse;
    int tag;
    int n_points;               // size of the point set rmse is the mean over (sncal_camera.n_points); set wherever rmse is
};

__device__ __forceinline__ void cam_set_pose(Cam& c, const double* R, const double* t) {   // position = -R^T t
#pragma unroll
    for (int i = 0; i < 9; ++i) c.R[i] = R[i];
    c.pos[0] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
    c.pos[1] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
    c.pos[2] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
}
__device__ __forceinline__ void cam_t(const Cam& c, double* t) {   // t = -R pos
    t[0] = -(c.R[0] * c.pos[0] + c.R[1] * c.pos[1] + c.R[2] * c.pos[2]);
    t[1] = -(c.R[3] * c.pos[0] + c.R[4] * c.pos[1] + c.R[5] * c.pos[2]);
    t[2] = -(c.R[6] * c.pos[0] + c.R[7] * c.pos[1] + c.R[8] * c.pos[2]);
}

struct Pts {   // lane-local point data
    double X64[3], X32[3];
    double u, v, u32, v32;
    int sched;       // SCHED_OPENCV / SCHED_CONVERGED
    int refine_iters;   // cap of refine_camera's LMSolver run (sncal_voter_cfg.refine_max_iters)
};

__device__ bool cam_solve_pnp(Cam& c, u64 mask, const Pts& p) {
    double R[9], t[3];
    const K4 k{c.fx, c.fy, c.cx, c.cy};
    if (!pnp_ransac(p.sched, mask, mask & GROUND_MASK, k, p.X64, p.u, p.v, R, t)) return false;
    cam_set_pose(c, R, t);
    return true;
}
__device__ void cam_refine(Cam& c, u64 mask, const Pts& p) {
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = c.R[i];
    cam_t(c, t);
    const K4 k{c.fx, c.fy, c.cx, c.cy};
    if (p.sched == SCHED_OPENCV) lm_solver_pose_auto(mask, R, t, k, p.X64, p.u, p.v, p.refine_iters, 1e-5);      // camera.py:116-117
    else refine_pose_lm(mask, R, t, k, p.X64, p.u, p.v, 100, 1e-10);
    cam_set_pose(c, R, t);
}
// Camera.projection_rmse (camera.py:270-277; project_point :249-268 with the fp32 round trip of distort :247)
__device__ double cam_rmse(const Cam& c, u64 mask, const Pts& p) {
    const int lane = threadIdx.x & 63;
    const double d[3] = {p.X64[0] - c.pos[0], p.X64[1] - c.pos[1], p.X64[2] - c.pos[2]};
    double r[3];
    mul3v(c.R, d, r);
    double px = 0, py = 0;
    if (!(r[2] <= 1e-3)) {
        const float xn = (float)(r[0] / r[2]), yn = (float)(r[1] / r[2]);
        px = (double)xn * c.fx + c.ppx;
        py = (double)yn * c.fy + c.ppy;
    }
    const double l2 = sqrt((p.u - px) * (p.u - px) + (p.v - py) * (p.v - py));
    return wsum(((mask >> lane) & 1) ? l2 : 0.0) / (double)popc64(mask);
}
__device__ __forceinline__ bool good_camera(const Cam& c) {   // prediction.py:469-484
    return c.fx >= 10 && c.fx <= 20000 && c.pos[0] > -250 && c.pos[0] < 250 && c.pos[1] > -250 && c.pos[1] < 250 &&
           c.pos[2] > -100 && c.pos[2] < 0;
}

__device__ int build_views(u64 mask, int min_pts, bool duplicate, View* views) {
    int nv = 0;
    const u64 pm[3] = {mask & GROUND_MASK, mask & GOAL_LEFT_MASK, mask & GOAL_RIGHT_MASK};
    for (int pl = 0; pl < 3; ++pl) {
        if (!pm[pl]) continue;
        double mult = 1.0;
        if (duplicate) {   // quirk Q1: the list object is appended once per id from the first detected one on
            int first = 0, len = 0;
            if (pl == 0) {
                len = 54;                                            // range(58) minus the 4 crossbar ids (Q6)
                const int id = __ffsll((long long)pm[0]) - 1;
                first = id - popc64(TOP_GATES_MASK & ((1ull << id) - 1));
            } else {
                len = 10;
                const int* ids = pl == 1 ? c_goal_left_ids : c_goal_right_ids;
                first = 10;
                for (int q = 9; q >= 0; --q) if ((pm[pl] >> ids[q]) & 1) first = q;
            }
            mult = (double)(len - first);
        }
        if (popc64(pm[pl]) >= min_pts) { views[nv].mask = pm[pl]; views[nv].kind = pl == 0 ? 0 : 1; views[nv].weight = mult; ++nv; }
    }
    return nv;
}

__device__ void cam_from_calibration(Cam& c, double f, const double* R0, const double* t0, int img_w, int img_h) {
    c.fx = c.fy = f;
    c.cx = (img_w - 1) * 0.5; c.cy = (img_h - 1) * 0.5;
    c.ppx = img_w / 2.0; c.ppy = img_h / 2.0;
    cam_set_pose(c, R0, t0);
}

enum { ST_OK = 0, ST_NONE = 1, ST_RAISE = 2 };   // value / None / exception

// prediction.py:487-520
__device__ int camera_from_homography(u64 mask, const Pts& p, int img_w, int img_h, Cam& c) {
    const u64 g = mask & GROUND_MASK;
    if (popc64(g) < 4) return ST_NONE;
    double H[9];
    if (!homography_ransac(g, p.X32[0], p.X32[1], p.u32, p.v32, 10.0, H)) return ST_NONE;
    double fx, fy;
    if (k_from_homography(H, img_w / 2.0, img_h / 2.0, fx, fy)) {
        c.fx = fx; c.fy = fy; c.cx = img_w / 2.0; c.cy = img_h / 2.0; c.ppx = c.cx; c.ppy = c.cy;
    } else {
        // prediction.py:514 ignores the failure flag of estimate_calibration_matrix_from_plane_homography: the Camera() keeps its
        // initial state -- calibration = eye(3), focal lengths 1 (camera.py:33-40), principal point (w/2, h/2) for project_point -- and
        // goes through solve_pnp / refine_camera / projection_rmse like any other.  Followed since round 4 (rounds 1-3 returned None
        // here): the K = I camera itself never survives the rmse tests of its callers, but a solve_pnp failure under it raises, and
        // the reference then has no camera for the frame.
        c.fx = c.fy = 1.0; c.cx = c.cy = 0.0; c.ppx = img_w / 2.0; c.ppy = img_h / 2.0;
    }
#ifdef SNCAL_SOLVE_TIMING
    const unsigned long long th0 = __builtin_amdgcn_s_memtime();
#endif
    if (!cam_solve_pnp(c, mask, p)) return ST_RAISE;
#ifdef SNCAL_SOLVE_TIMING
    const unsigned long long th1 = __builtin_amdgcn_s_memtime();
#endif
    cam_refine(c, mask, p);
#ifdef SNCAL_SOLVE_TIMING
    if ((threadIdx.x & 63) == 0) printf("  hom wave %d: solve_pnp %llu clk refine %llu clk fx %g\n", (int)(threadIdx.x >> 6), th1 - th0, __builtin_amdgcn_s_memtime() - th1, c.fx);
#endif
    c.rmse = cam_rmse(c, mask, p); c.n_points = popc64(mask);
    return ST_OK;
}

// prediction.py:523-555 + get_camera_gen :609-640 (exceptions inside are swallowed -> None)
__device__ int camera_all_points(u64 mask, const Pts& p, int img_w, int img_h, Cam& c) {
    View views[3];
    const int nv = build_views(mask, 6, true, views);
    double total = 0;
    for (int i = 0; i < nv; ++i) total += views[i].weight * popc64(views[i].mask);
    if (!(nv > 0 && total > 6)) return ST_NONE;
    double f, R0[9], t0[3];
#ifdef SNCAL_SOLVE_TIMING
    unsigned long long tq = __builtin_amdgcn_s_memtime();
#define CAP_LAP(fmt, ...) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); if ((threadIdx.x & 63) == 0) printf("  cap wave %d: " fmt "\n", (int)(threadIdx.x >> 6), tn_ - tq, ##__VA_ARGS__); tq = tn_; } while (0)
#else
#define CAP_LAP(...) do {} while (0)
#endif
    const bool cal_ok = calibrate_planes(p.sched, views, nv, p.X32, p.u32, p.v32, img_w, img_h, f, R0, t0);
    CAP_LAP("calibrate_planes %llu clk npts %d nviews %d ok %d f %g", popc64(mask), nv, (int)cal_ok, cal_ok ? f : 0.0);
    if (!cal_ok) return ST_NONE;
    cam_from_calibration(c, f, R0, t0, img_w, img_h);
    const bool pnp_ok = cam_solve_pnp(c, mask, p);            // always runs (quirk Q2)
    CAP_LAP("solve_pnp %llu clk ok %d", (int)pnp_ok);
    if (!pnp_ok) return ST_NONE;
    // Same outcome, less work (shared with oracle/solve.py): every caller keeps this camera only if good_camera accepts it, and the
    // focal-length clause does not depend on the pose -- a candidate calibrated outside [10, 20000] px is discarded whatever
    // refine_camera does to it, so it is not refined (under f ~ 0.04 px the reference's 20000-iteration LM runs to the end: 100 ms of
    // one wavefront for a camera nobody uses, which is what the 200-iteration cap of rounds 1-3 was for)
    if (popc64(mask) > 6 && c.fx >= 10 && c.fx <= 20000) cam_refine(c, mask, p);
    CAP_LAP("refine %llu clk");
    c.rmse = cam_rmse(c, mask, p); c.n_points = popc64(mask);
    return ST_OK;
}

// prediction.py:572-606
__device__ int camera_accurate_points(u64 mask, const Pts& p, double thr, int img_w, int img_h, Cam& c) {
    const int lane = threadIdx.x & 63;
    const u64 g = mask & GROUND_MASK;
    if (popc64(g) < 4) return ST_NONE;
    double H[9];
    if (!homography_ransac(g, p.X32[0], p.X32[1], p.u32, p.v32, thr, H)) return ST_NONE;
    double pu, pv;
    apply_h(H, p.X32[0], p.X32[1], pu, pv);
    const double err = sqrt((pu - p.u32) * (pu - p.u32) + (pv - p.v32) * (pv - p.v32));
    const u64 sel = __ballot(((g >> lane) & 1) && err < thr) | (mask & TOP_GATES_MASK);
    return camera_all_points(sel, p, img_w, img_h, c);
}

__device__ u64 add_line_points(u64 mask, Pts& p, const float* line_pts, const sncal_voter_cfg& cfg, int mode,
                               int n_ground_kp) {
    // prediction.py:186-192 (mode 2), :270-278 (mode 1, voter), :356-364 (mode 0, original_voter)
    if (!line_pts) return mask;
    const int lane = threadIdx.x & 63;
    for (int i = 0; i < 30; ++i) {
        const float lx = line_pts[i * 3 + 0], ly = line_pts[i * 3 + 1], valid = line_pts[i * 3 + 2];
        if (!(valid > 0.5f) || ((mask >> i) & 1)) continue;
        bool take;
        if (mode == 0) take = n_ground_kp < cfg.min_points_per_plane || (0 <= lx && lx <= cfg.img_w && 0 <= ly && ly <= cfg.img_h);
        else if (mode == 1) take = popc64(mask & GROUND_MASK) < cfg.min_points_per_plane;
        else take = popc64(mask) <= cfg.min_points;
        if (take) {
            mask |= 1ull << i;
            if (lane == i) { p.u = (double)lx; p.v = (double)ly; p.u32 = (double)lx; p.v32 = (double)ly; }
        }
    }
    return mask;
}

__device__ u64 select_points(const float conf, double thr, bool reliable_rule, int reliable_thresh) {
    const int lane = threadIdx.x & 63;
    const bool det = lane < NPTS && (double)conf > thr;
    const u64 dm = __ballot(det);
    if (!reliable_rule) return dm;
    // n_det_points (prediction.py:178, 345) compares the float32 COLUMN with the python float: under the reference's numpy (1.24) that is a
    // float32 comparison, unlike the per-point test above (a float32 scalar: double) -- a confidence of exactly float32(0.2) is a point
    // but does not count here
    const int n_det = popc64(__ballot(lane < NPTS && conf > (float)thr));
    return n_det < reliable_thresh ? dm : dm & KEEP_MASK;
}

// prediction.py:339-437, in the three pieces calibrate_kernel runs on two wavefronts (the homography camera and the calibrated camera are
// independent solves of the same points; the reference builds them one after the other):
//   ov_points   the selection (:345-357)                                  -> mask, and the line points in p
//   ov_hom      camera_from_homography (:359)                             -> hs, hom
//   ov_cal      the multi-plane calibration branch (:361-420)             -> ST_RAISE / ST_OK (a camera, refined) / ST_NONE
//   ov_combine  the reference's order of precedence (:359-437): an exception of either half leaves, the calibrated camera wins, the
//               homography camera is the fallback below rmse 26
__device__ u64 ov_points(const float* kp, const float* line_pts, const sncal_voter_cfg& cfg, double thr, Pts& p) {
    const u64 mask = select_points(kp[2], thr, true, cfg.reliable_thresh);
    return add_line_points(mask, p, line_pts, cfg, 0, popc64(mask & GROUND_MASK));
}
__device__ int ov_cal(u64 mask, const sncal_voter_cfg& cfg, const Pts& p, Cam& out) {
    View views[3];
    const int nv = build_views(mask, cfg.min_points_per_plane, false, views);
    if (!(nv > 0 && popc64(mask) > cfg.min_points)) return ST_NONE;
    double f, R0[9], t0[3];
    if (!calibrate_planes(p.sched, views, nv, p.X32, p.u32, p.v32, cfg.img_w, cfg.img_h, f, R0, t0)) return ST_RAISE;
    cam_from_calibration(out, f, R0, t0, cfg.img_w, cfg.img_h);
    out.tag = SNCAL_CAM_ORIGINAL;
    if (popc64(mask & GROUND_MASK) < cfg.min_points_per_plane && !cam_solve_pnp(out, mask, p)) return ST_RAISE;
    if (!good_camera(out)) return ST_NONE;
    if (popc64(mask) > cfg.min_points_for_refinement) cam_refine(out, mask, p);
    return ST_OK;
}
__device__ int ov_combine(u64 mask, const Pts& p, int hs, const Cam& hom, int cs, const Cam& cal, Cam& out) {
    if (hs == ST_RAISE || cs == ST_RAISE) return ST_RAISE;      // (the serial order raises in the homography half first: same outcome)
    if (cs == ST_OK) out = cal;
    else if (hs == ST_OK && hom.rmse < 26) { out = hom; out.tag = SNCAL_CAM_ORIGINAL_HOM; }
    else return ST_NONE;
    out.rmse = cam_rmse(out, mask, p); out.n_points = popc64(mask);
    return ST_OK;
}

// prediction.py:259-330
// the final choice among the homography camera and the four subset cameras (prediction.py:293-329)
__device__ int voter_select(const sncal_voter_cfg& cfg, int hs, const Cam& hom, const int (&st)[4], const Cam (&cands)[4], Cam& out) {
    if (hs == ST_RAISE) return ST_RAISE;
    const int tags[4] = {SNCAL_CAM_VOTER_REL, SNCAL_CAM_VOTER_ACC, SNCAL_CAM_VOTER_ALL, SNCAL_CAM_VOTER_GROUND};
    int best = -1;
    bool best_flag = false;
    double best_inv = 0;
    for (int i = 0; i < 4; ++i) {          // python max(): first maximum of (flag, 1/rmse) in list order
        if (st[i] != ST_OK || !good_camera(cands[i])) continue;
        if (cands[i].rmse == 0.0) return ST_RAISE;                    // 1/0 -> ZeroDivisionError (quirk Q5)
        const bool flag = i == 0 && cands[i].rmse < cfg.max_rmse_rel;
        const double inv = 1.0 / cands[i].rmse;
        if (best < 0 || (flag && !best_flag) || (flag == best_flag && inv > best_inv)) { best = i; best_flag = flag; best_inv = inv; }
    }
    if (best >= 0 && cands[best].rmse < cfg.max_rmse) { out = cands[best]; out.tag = tags[best]; return ST_OK; }
    if (hs == ST_OK && hom.rmse < cfg.max_rmse) { out = hom; out.tag = SNCAL_CAM_VOTER_HOM; return ST_OK; }
    return ST_NONE;
}

// voter_select's choice as an INDEX, on the numbers it reads alone (sncal_calibrate_sweep: one solve, many (max_rmse, max_rmse_rel)):
// 0..3 = cands[i] (rel, acc, all, ground), 4 = the homography camera, -1 = no camera, -2 = the voter raises.  ok bit i: cands[i] was
// solved and is a good_camera; bit 4: the homography camera was solved.  Same comparisons in the same order as voter_select above;
// tests/test_sweep_gpu.py holds the two together byte for byte.
enum { PICK_HOM = 4, PICK_NONE = -1, PICK_RAISE = -2 };
__device__ __forceinline__ int voter_pick(double max_rmse, double max_rmse_rel, bool hom_raises, unsigned ok, const double (&rmse)[5]) {
    if (hom_raises) return PICK_RAISE;
    int best = -1;
    bool best_flag = false;
    double best_inv = 0;
    for (int i = 0; i < 4; ++i) {
        if (!((ok >> i) & 1)) continue;
        if (rmse[i] == 0.0) return PICK_RAISE;
        const bool flag = i == 0 && rmse[i] < max_rmse_rel;
        const double inv = 1.0 / rmse[i];
        if (best < 0 || (flag && !best_flag) || (flag == best_flag && inv > best_inv)) { best = i; best_flag = flag; best_inv = inv; }
    }
    if (best >= 0 && rmse[best] < max_rmse) return best;
    if (((ok >> PICK_HOM) & 1) && rmse[PICK_HOM] < max_rmse) return PICK_HOM;
    return PICK_NONE;
}

// (noinline: calibrate_kernel calls it in one place, and inlined there its five cameras share the register allocation of the kernel's other
// algorithms -- the kernel's own spills went from 117 to 1778 VGPRs.  As a function it compiles to what it was with two call sites.)
__device__ __attribute__((noinline)) int voter(const float* kp, const float* line_pts, const sncal_voter_cfg& cfg, double thr, Pts p, Cam& out) {
    u64 mask = select_points(kp[2], thr, false, 0);
    mask = add_line_points(mask, p, line_pts, cfg, 1, 0);
    Cam hom;
    const int hs = camera_from_homography(mask, p, cfg.img_w, cfg.img_h, hom);
    if (hs == ST_RAISE) return ST_RAISE;
    Cam cands[4];
    int st[4];
    st[2] = camera_all_points(mask, p, cfg.img_w, cfg.img_h, cands[2]);
    st[0] = camera_all_points(mask & KEEP_MASK, p, cfg.img_w, cfg.img_h, cands[0]);
    st[1] = camera_accurate_points(mask, p, 5.0, cfg.img_w, cfg.img_h, cands[1]);
    st[3] = camera_all_points(mask & GROUND_MASK, p, cfg.img_w, cfg.img_h, cands[3]);
    return voter_select(cfg, hs, hom, st, cands, out);
}

// The same voter spread over the four waves of a workgroup: its five cameras are independent solves of the same
// points (prediction.py:281-291 builds them one after the other), so wave 0 takes the homography camera and the
// ground-plane subset, waves 1..3 the all / reliable / H-consistent subsets; every wave then runs the (cheap) selection
// on the five results in LDS.  Each camera is computed by the same code on the same inputs as in voter(): identical bits.
struct VoterShared { Cam hom; Cam cands[4]; int hs; int st[4]; };

__device__ int voter_parallel(const float* kp, const float* line_pts, const sncal_voter_cfg& cfg, double thr, Pts p, VoterShared& sh,
                              Cam& out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u64 mask = select_points(kp[2], thr, false, 0);
    mask = add_line_points(mask, p, line_pts, cfg, 1, 0);
    Cam c;
    c.tag = SNCAL_CAM_NONE;
    if (wave == 0) {
        const int hs = camera_from_homography(mask, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.hom = c; sh.hs = hs; }
        const int s3 = camera_all_points(mask & GROUND_MASK, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.cands[3] = c; sh.st[3] = s3; }
    } else if (wave == 1) {
        const int s2 = camera_all_points(mask, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.cands[2] = c; sh.st[2] = s2; }
    } else if (wave == 2) {
        const int s0 = camera_all_points(mask & KEEP_MASK, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.cands[0] = c; sh.st[0] = s0; }
    } else {
        const int s1 = camera_accurate_points(mask, p, 5.0, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.cands[1] = c; sh.st[1] = s1; }
    }
    __syncthreads();
    const int r = voter_select(cfg, sh.hs, sh.hom, sh.st, sh.cands, out);
    __syncthreads();                                   // everyone has read the results before the next pass overwrites them
    return r;
}

// prediction.py:138-170
__device__ int opencv_calibration(const float* kp, const sncal_voter_cfg& cfg, const Pts& p, Cam& out) {
    const int lane = threadIdx.x & 63;
    const u64 mask = __ballot(lane < NPTS && (double)kp[2] > cfg.conf_thresh) & GROUND_MASK;
    if (popc64(mask) <= 5) return ST_NONE;
    View v{mask, 0, 1.0};
    double f, R0[9], t0[3];
    if (!calibrate_planes(p.sched, &v, 1, p.X32, p.u32, p.v32, cfg.img_w, cfg.img_h, f, R0, t0)) return ST_RAISE;
    cam_from_calibration(out, f, R0, t0, cfg.img_w, cfg.img_h);
    out.tag = SNCAL_CAM_ORIGINAL;
    out.rmse = cam_rmse(out, mask, p); out.n_points = popc64(mask);
    return ST_OK;
}

// prediction.py:172-243
__device__ int opencv_calibration_multiplane(const float* kp, const float* line_pts, const sncal_voter_cfg& cfg, Pts p, Cam& out) {
    u64 mask = select_points(kp[2], cfg.conf_thresh, true, cfg.reliable_thresh);
    mask = add_line_points(mask, p, line_pts, cfg, 2, 0);
    View views[3];
    const int nv = build_views(mask, cfg.min_points_per_plane, false, views);
    if (!(nv > 0 && popc64(mask) > cfg.min_points)) return ST_NONE;
    double f, R0[9], t0[3];
    if (!calibrate_planes(p.sched, views, nv, p.X32, p.u32, p.v32, cfg.img_w, cfg.img_h, f, R0, t0)) return ST_RAISE;
    if (!(f > cfg.min_focal_length)) return ST_NONE;
    cam_from_calibration(out, f, R0, t0, cfg.img_w, cfg.img_h);
    if (popc64(mask) > cfg.min_points_for_refinement) cam_refine(out, mask, p);
    out.tag = SNCAL_CAM_ORIGINAL;
    out.rmse = cam_rmse(out, mask, p); out.n_points = popc64(mask);
    return ST_OK;
}

__device__ void load_points(const float* kp, Pts& p) {
    const int lane = threadIdx.x & 63;
    const int id = lane < NPTS ? lane : 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) { p.X64[i] = c_P64[id * 3 + i]; p.X32[i] = c_P32[id * 3 + i]; }
    p.u = (double)kp[0]; p.v = (double)kp[1];      // float(pred[i,0]) -> python float; float32 -> float64 is exact
    p.u32 = p.u; p.v32 = p.v;
}

}  // namespace
