// Batched camera solve on gfx950: one 64-lane wavefront per frame.
//
// The solvers and the reference's control flow are in solve_*.hpp (wave, linalg, homography, pose, calib, flow), included below and by
// this file alone; here: the point-id masks and tables, the kernels, the pitch upload, the scratch cache and the C entry points.
//
// Mapping to the hardware: lane i owns keypoint id i (57 template points <= 64 lanes; a line-intersection
// candidate fills the slot of a missing keypoint with the same id, prediction.py:356-364).  A point subset
// is a 64-bit lane mask.  Everything per point (residuals, Jacobian rows, inlier tests) is lane-parallel;
// normal equations are assembled with butterfly wave reductions (every lane ends with bit-identical sums,
// so all control flow stays wave-uniform); the small dense algebra (8x8 / 6x6 Cholesky, 3x3 adjugates,
// polar iteration) runs redundantly in every lane's registers.  RANSAC hypotheses are lane-parallel too:
// each lane draws its own 4-point sample with a counter-based hash and scores it against all points.
// All arithmetic is fp64.  The solve is latency-bound (~1e5 FLOP per frame): it is reported in frames/s,
// not as a roofline fraction, and runs on its own stream beside the MFMA-bound network.
#include "common.hpp"
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>

namespace {

constexpr int NPTS = 57;
constexpr unsigned long long TOP_GATES_MASK = (1ull << 0) | (1ull << 1) | (1ull << 24) | (1ull << 25);
constexpr unsigned long long ALL_MASK = (1ull << NPTS) - 1;
constexpr unsigned long long GROUND_MASK = ALL_MASK & ~TOP_GATES_MASK;
// prediction.py:20-21, 25-26
constexpr unsigned long long GOAL_LEFT_MASK = (1ull << 0) | (1ull << 1) | (1ull << 2) | (1ull << 3) | (1ull << 6) |
                                              (1ull << 7) | (1ull << 10) | (1ull << 11) | (1ull << 12) | (1ull << 13);
constexpr unsigned long long GOAL_RIGHT_MASK = (1ull << 18) | (1ull << 19) | (1ull << 22) | (1ull << 23) | (1ull << 24) |
                                               (1ull << 25) | (1ull << 26) | (1ull << 27) | (1ull << 28) | (1ull << 29);
constexpr unsigned long long KEEP_MASK = ((1ull << 29) - 1) | (1ull << 40) | (1ull << 41) | (1ull << 42) | (1ull << 44) |
                                         (1ull << 45) | (1ull << 48) | (1ull << 51) | (1ull << 52) | (1ull << 55);

__constant__ double c_P64[NPTS * 3];
__constant__ double c_P32[NPTS * 3];
// order of ids inside the goal-plane id lists (for the duplication multiplicity, quirk Q1)
__constant__ int c_goal_left_ids[10] = {0, 1, 2, 3, 6, 7, 10, 11, 12, 13};
__constant__ int c_goal_right_ids[10] = {18, 19, 22, 23, 24, 25, 26, 27, 28, 29};

typedef unsigned long long u64;

}  // namespace

#include "solve_wave.hpp"
#include "solve_linalg.hpp"
#include "solve_homography.hpp"
#include "solve_pose.hpp"
#include "solve_calib.hpp"
#include "solve_flow.hpp"

namespace {

// Four wavefronts per workgroup (calibrate_kernel: four frames, or two frames x two cameras): a solver wave owns a whole SIMD register
// file (512 VGPRs), so a lone wave per CU would keep the co-running convolution workgroups (one wave on each SIMD) off that CU; packed,
// 64 frames block 16-32 CUs instead of degrading 64.
constexpr int STATUS_PENDING = -1;      // iterative_voter frames whose original_voter pass found no camera: left for voter_kernel

__device__ __forceinline__ void store_camera(sncal_camera* out, int st, const Cam& cam) {
    sncal_camera o;
    memset(&o, 0, sizeof(o));
    if (st == ST_OK) {
        for (int i = 0; i < 3; ++i) o.position[i] = cam.pos[i];
        for (int i = 0; i < 9; ++i) o.rotation[i] = cam.R[i];
        o.fx = cam.fx; o.fy = cam.fy; o.cx = cam.cx; o.cy = cam.cy; o.rmse = cam.rmse;
        o.status = cam.tag; o.n_points = cam.n_points;
    }
    *out = o;
}

// The prologue of every kernel that solves a frame: the lane's keypoint (confidence -1 = absent: lanes past the template, and every lane
// when `valid` is false -- a wave of calibrate_kernel's last workgroup without a frame), the frame's line points, the template points and
// the minimiser settings of the call
__device__ __forceinline__ void load_frame(const float* kpts, const float* line_pts, int frame, bool valid, const sncal_voter_cfg& cfg,
                                           float (&kp)[3], const float*& lp, Pts& p) {
    const int lane = threadIdx.x & 63;
    kp[0] = 0.f; kp[1] = 0.f; kp[2] = -1.f;
    if (valid && lane < NPTS) {
        const float* src = kpts + ((size_t)frame * NPTS + lane) * 3;
        kp[0] = src[0]; kp[1] = src[1]; kp[2] = src[2];
    }
    lp = line_pts && valid ? line_pts + (size_t)frame * 90 : nullptr;
    load_points(kp, p);
    p.sched = cfg.lm_schedule == 1 ? SCHED_CONVERGED : SCHED_OPENCV;
    p.refine_iters = cfg.refine_max_iters > 0 ? cfg.refine_max_iters : 20000;
}

// iterative_voter's second half (prediction.py:250-256) for the frames calibrate_kernel left pending: one workgroup per
// frame, the voter's five cameras on four waves.  Frames that already have a camera leave at once.
__global__ __launch_bounds__(256, 1) void voter_kernel(const float* __restrict__ kpts, const float* __restrict__ line_pts, int B,
                                                       sncal_voter_cfg cfg, sncal_camera* __restrict__ out) {
    __shared__ VoterShared sh;
    const int frame = blockIdx.x;
    if (out[frame].status != STATUS_PENDING) return;
    float kp[3];
    const float* lp;
    Pts p;
    load_frame(kpts, line_pts, frame, true, cfg, kp, lp, p);
    Cam cam;
    cam.tag = SNCAL_CAM_NONE;
    int st = ST_NONE;
    for (int i = 0; i < cfg.n_conf_threshs; ++i) {
        st = voter_parallel(kp, lp, cfg, cfg.conf_threshs[i], p, sh, cam);
        if (st != ST_NONE) break;                      // camera found, or an exception leaves iterative_voter
    }
    if (threadIdx.x == 0) store_camera(out + frame, st, cam);
}

// The same second half with ONE WAVEFRONT PER CAMERA (round 4).  A frame that ends without a camera walks all of iterative_voter's
// thresholds, and every threshold costs the voter's five cameras: on voter_kernel's four waves (wave 0 owns two cameras) the bench's
// slowest frame took 2 x 5.9 ms = the whole 11.7 ms of the launch -- eight weak points, f = 53 px, every camera 1.1 ms of
// calibrate_planes + 0.6 ms of RANSAC PnP + 2 ms of refine_camera at the bench's 200-iteration cap.  The cameras of ALL thresholds are
// independent of each other (prediction.py:250-256 only stops at the first threshold that yields one; what a threshold computes does
// not depend on the thresholds before it), so they are computed side by side, threshold x camera = up to 15 wavefronts per pending
// frame, each on the code and the inputs the serial voter gives it (identical bits), and voter_select_kernel then walks the thresholds
// in the reference's order and keeps the first result that is not "no camera".  Wall time = the slowest single camera (3.8 ms on
// that frame); the work of thresholds behind the deciding one is wasted CU time on a few wavefronts.
enum { VT_HOM = 0, VT_GROUND = 1, VT_ALL = 2, VT_KEEP = 3, VT_ACC = 4, VT_TASKS = 5 };
__global__ __launch_bounds__(64, 1) void voter_task_kernel(const float* __restrict__ kpts, const float* __restrict__ line_pts, int B,
                                                           sncal_voter_cfg cfg, const sncal_camera* __restrict__ out, VoterShared* __restrict__ slots) {
    const int task = (int)blockIdx.x % VT_TASKS, ti = ((int)blockIdx.x / VT_TASKS) % cfg.n_conf_threshs;
    const int frame = (int)blockIdx.x / (VT_TASKS * cfg.n_conf_threshs);
    if (frame >= B || out[frame].status != STATUS_PENDING) return;
    const int lane = threadIdx.x & 63;
    float kp[3];
    const float* lp;
    Pts p;
    load_frame(kpts, line_pts, frame, true, cfg, kp, lp, p);
    u64 mask = select_points(kp[2], cfg.conf_threshs[ti], false, 0);
    mask = add_line_points(mask, p, lp, cfg, 1, 0);
    VoterShared& sh = slots[(size_t)frame * cfg.n_conf_threshs + ti];
    Cam c;
    c.tag = SNCAL_CAM_NONE;
    if (task == VT_HOM) {
        const int hs = camera_from_homography(mask, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { sh.hom = c; sh.hs = hs; }
    } else {
        int s = ST_NONE, slot = 0;
        if (task == VT_GROUND) { s = camera_all_points(mask & GROUND_MASK, p, cfg.img_w, cfg.img_h, c); slot = 3; }
        else if (task == VT_ALL) { s = camera_all_points(mask, p, cfg.img_w, cfg.img_h, c); slot = 2; }
        else if (task == VT_KEEP) { s = camera_all_points(mask & KEEP_MASK, p, cfg.img_w, cfg.img_h, c); slot = 0; }
        else { s = camera_accurate_points(mask, p, 5.0, cfg.img_w, cfg.img_h, c); slot = 1; }
        if (lane == 0) { sh.cands[slot] = c; sh.st[slot] = s; }
    }
}

// prediction.py:250-256 on the cameras voter_task_kernel left: thresholds in order, the first one whose voter returns a camera (or raises)
// ends the frame.  One thread per frame (the selection is scalar code).
__global__ __launch_bounds__(64) void voter_select_kernel(int B, sncal_voter_cfg cfg, const VoterShared* __restrict__ slots, sncal_camera* __restrict__ out) {
    const int frame = (int)(blockIdx.x * 64 + threadIdx.x);
    if (frame >= B || out[frame].status != STATUS_PENDING) return;
    Cam cam;
    cam.tag = SNCAL_CAM_NONE;
    int st = ST_NONE;
    for (int i = 0; i < cfg.n_conf_threshs; ++i) {
        const VoterShared& sh = slots[(size_t)frame * cfg.n_conf_threshs + i];
        st = voter_select(cfg, sh.hs, sh.hom, sh.st, sh.cands, cam);
        if (st != ST_NONE) break;
    }
    store_camera(out + frame, st, cam);
}

// ---- sncal_calibrate_sweep: one solve, every (max_rmse, max_rmse_rel) ------------------------------------------------------------------
// The two parameters are read by voter_select alone: what the first pass and voter_task_kernel compute does not depend on them.  A frame
// therefore has at most S = 1 + 5 T distinct cameras (the first pass's, and five per threshold), and a grid point is a choice among
// them.  sweep_outcomes_kernel writes them as the records store_camera would write had the selection taken them, plus the few numbers the
// selection reads (SweepCand); sweep_select_kernel is voter_select_kernel's walk over the thresholds per (grid point, frame).
struct SweepCand { double rmse[5]; unsigned ok; int raises; };      // rel, acc, all, ground, hom of one (frame, threshold): voter_pick's inputs

// the voter of this threshold raises whatever the two parameters are: voter_select's two ST_RAISE exits
__device__ __forceinline__ bool voter_raises(const VoterShared& sh) {
    if (sh.hs == ST_RAISE) return true;
    for (int i = 0; i < 4; ++i)
        if (sh.st[i] == ST_OK && good_camera(sh.cands[i]) && sh.cands[i].rmse == 0.0) return true;
    return false;
}

// voter (algorithm 2) has no first pass: every frame goes to the task stage
__global__ __launch_bounds__(64) void sweep_mark_pending_kernel(int B, sncal_camera* __restrict__ first) {
    const int frame = (int)(blockIdx.x * 64 + threadIdx.x);
    if (frame >= B) return;
    Cam none;
    none.tag = SNCAL_CAM_NONE;
    store_camera(first + frame, ST_NONE, none);
    first[frame].status = STATUS_PENDING;
}

// One thread per (frame, 0 = first pass | 1 + t = threshold t).  A slot no grid point can take is the all-zero record: a solve that failed,
// a camera good_camera refuses, every slot of a threshold that raises or lies behind one that does, and the voter slots of a frame the
// first pass settled (their VoterShared was never written).
__global__ __launch_bounds__(64) void sweep_outcomes_kernel(int B, int T, const sncal_camera* __restrict__ first, const VoterShared* __restrict__ slots,
                                                            sncal_camera* __restrict__ outcomes, SweepCand* __restrict__ cands) {
    const int i = (int)(blockIdx.x * 64 + threadIdx.x), frame = i / (T + 1), j = i % (T + 1);
    if (frame >= B) return;
    const size_t S = 1 + 5 * (size_t)T;
    const bool pending = first[frame].status == STATUS_PENDING;
    Cam none;
    none.tag = SNCAL_CAM_NONE;
    if (j == 0) {
        if (pending) store_camera(outcomes + frame * S, ST_NONE, none);
        else outcomes[frame * S] = first[frame];
        return;
    }
    const int t = j - 1;
    sncal_camera* const o = outcomes + frame * S + 1 + 5 * t;
    SweepCand sc;
    for (int k = 0; k < 5; ++k) sc.rmse[k] = 0.0;
    sc.ok = 0; sc.raises = 0;
    bool open = pending;                                   // some grid point may reach this threshold
    for (int q = 0; q < t && open; ++q) open = !voter_raises(slots[(size_t)frame * T + q]);
    if (open && voter_raises(slots[(size_t)frame * T + t])) { sc.raises = 1; open = false; }
    const int tags[4] = {SNCAL_CAM_VOTER_REL, SNCAL_CAM_VOTER_ACC, SNCAL_CAM_VOTER_ALL, SNCAL_CAM_VOTER_GROUND};
    for (int k = 0; k < 5; ++k) {
        bool ok = false;
        if (open) {
            const VoterShared& sh = slots[(size_t)frame * T + t];
            ok = k < 4 ? (sh.st[k] == ST_OK && good_camera(sh.cands[k])) : sh.hs == ST_OK;
            if (ok) {
                Cam c = k < 4 ? sh.cands[k] : sh.hom;
                c.tag = k < 4 ? tags[k] : SNCAL_CAM_VOTER_HOM;
                store_camera(o + k, ST_OK, c);
                sc.rmse[k] = c.rmse; sc.ok |= 1u << k;
            }
        }
        if (!ok) store_camera(o + k, ST_NONE, none);
    }
    cands[(size_t)frame * T + t] = sc;
}

// One thread per (grid point, frame), frame fastest: a wavefront's 64 choices are 256 contiguous bytes of d_choice (n_grid, B).
__global__ __launch_bounds__(256) void sweep_select_kernel(int B, int T, int n_grid, const double* __restrict__ grid, const sncal_camera* __restrict__ first,
                                                           const SweepCand* __restrict__ cands, int32_t* __restrict__ choice) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n_grid * B) return;
    const int g = (int)(i / B), frame = (int)(i % B);
    const double max_rmse = grid[2 * g], max_rmse_rel = grid[2 * g + 1];
    const int fs = first[frame].status;
    int pick = fs > 0 ? 0 : -1;
    if (fs == STATUS_PENDING) {
        for (int t = 0; t < T; ++t) {                      // prediction.py:250-256: the first threshold with a camera, or an exception, ends the walk
            const SweepCand sc = cands[(size_t)frame * T + t];
            const int r = voter_pick(max_rmse, max_rmse_rel, sc.raises != 0, sc.ok, sc.rmse);
            if (r == PICK_NONE) continue;
            if (r >= 0) pick = 1 + 5 * t + r;
            break;
        }
    }
    choice[i] = pick;
}

// iterative_voter / original_voter (algorithms 0, 1): TWO wavefronts per frame, two frames per workgroup -- wave 2 i the homography
// camera, wave 2 i + 1 the calibrated camera of frame i (ov_hom / ov_cal above), the even wave combines them in the reference's order
// and, for iterative_voter, marks a frame without a camera pending for the voter stage.  The other algorithms: one wavefront per frame,
// four frames per workgroup.  The launcher sizes the grid accordingly.
struct OvHalf { Cam cam; int st; };
__global__ __launch_bounds__(256, 1) void calibrate_kernel(const float* __restrict__ kpts, const float* __restrict__ line_pts,
                                                           int B, sncal_voter_cfg cfg, sncal_camera* __restrict__ out, int defer_voter) {
    __shared__ OvHalf half[2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool paired = cfg.algorithm <= 1;
    const int frame = paired ? (int)blockIdx.x * 2 + (wave >> 1) : (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    const int role = paired ? wave & 1 : 0;
    const bool valid = frame < B;
    if (!paired && !valid) return;
    float kp[3];
    const float* lp;
    Pts p;
    load_frame(kpts, line_pts, frame, valid, cfg, kp, lp, p);
    Cam cam;
    cam.tag = SNCAL_CAM_NONE;
    int st = ST_NONE;
    if (paired) {
        u64 mask = 0;
        Cam hom;
        int hs = ST_NONE;
        if (valid) {
            mask = ov_points(kp, lp, cfg, cfg.algorithm == 0 ? 0.5 : cfg.conf_thresh, p);
            if (role == 1) {
                Cam cal;
                cal.tag = SNCAL_CAM_NONE;
                const int cs = ov_cal(mask, cfg, p, cal);
                if (lane == 0) { half[wave >> 1].cam = cal; half[wave >> 1].st = cs; }
            } else {
                hs = camera_from_homography(mask, p, cfg.img_w, cfg.img_h, hom);
            }
        }
        __syncthreads();
        if (!valid || role == 1) return;
        st = ov_combine(mask, p, hs, hom, half[wave >> 1].st, half[wave >> 1].cam, cam);
        if (cfg.algorithm == 0 && st != ST_OK) {   // iterative_voter, prediction.py:245-257
            if (defer_voter) {
                if (lane == 0) { store_camera(out + frame, ST_NONE, cam); out[frame].status = STATUS_PENDING; }
                return;
            }
            st = ST_NONE;   // not deferred = no thresholds (n_conf_threshs == 0): iterative_voter's loop is empty and leaves no camera
        }
    } else {
        switch (cfg.algorithm) {
            case 2: st = voter(kp, lp, cfg, cfg.conf_thresh, p, cam); break;
            case 3: st = opencv_calibration(kp, cfg, p, cam); break;
            default: st = opencv_calibration_multiplane(kp, lp, cfg, p, cam); break;
        }
    }
    if (lane == 0) store_camera(out + frame, st, cam);
}

// Round 5: the first pass as SINGLE-WAVE workgroups.  calibrate_kernel's paired form couples the two halves of a frame (and two frames)
// in one 256-thread workgroup through LDS and a barrier: a workgroup of four 512-register waves needs a completely free CU, and it
// keeps all four SIMDs until its slowest wave is through -- at the reference's refine criterion that can be a 330 ms Levenberg-Marquardt
// crawl.  On the CU-masked solve streams of the pipeline (8 CUs, pipeline.py) the crawling waves of earlier batches sit one per CU, no
// CU ever has four free SIMDs, and the next batch's first pass waited for them: the step went from 113 to 155 ms (measured).  Here every
// (frame, half) is a 64-thread workgroup that needs ONE free SIMD and leaves its result in a per-frame slot; first_pass_combine_kernel
// (one wave per frame, small) then applies the reference's order of precedence.  Same device functions on the same inputs as the
// paired form: identical bytes (tests/test_solve_gpu.py).
struct FirstPass { Cam hom; Cam cal; int hs; int cs; };
__global__ __launch_bounds__(64, 1) void first_pass_task_kernel(const float* __restrict__ kpts, const float* __restrict__ line_pts, int B,
                                                                sncal_voter_cfg cfg, FirstPass* __restrict__ fp) {
    const int frame = (int)blockIdx.x >> 1, role = (int)blockIdx.x & 1, lane = threadIdx.x & 63;
    if (frame >= B) return;
    float kp[3];
    const float* lp;
    Pts p;
    load_frame(kpts, line_pts, frame, true, cfg, kp, lp, p);
    const u64 mask = ov_points(kp, lp, cfg, cfg.algorithm == 0 ? 0.5 : cfg.conf_thresh, p);
    Cam c;
    c.tag = SNCAL_CAM_NONE;
    if (role == 1) {
        const int cs = ov_cal(mask, cfg, p, c);
        if (lane == 0) { fp[frame].cal = c; fp[frame].cs = cs; }
    } else {
        const int hs = camera_from_homography(mask, p, cfg.img_w, cfg.img_h, c);
        if (lane == 0) { fp[frame].hom = c; fp[frame].hs = hs; }
    }
}
__global__ __launch_bounds__(64) void first_pass_combine_kernel(const float* __restrict__ kpts, const float* __restrict__ line_pts, int B,
                                                                sncal_voter_cfg cfg, const FirstPass* __restrict__ fp,
                                                                sncal_camera* __restrict__ out, int defer_voter) {
    const int frame = (int)blockIdx.x, lane = threadIdx.x & 63;
    if (frame >= B) return;
    float kp[3];
    const float* lp;
    Pts p;
    load_frame(kpts, line_pts, frame, true, cfg, kp, lp, p);
    const u64 mask = ov_points(kp, lp, cfg, cfg.algorithm == 0 ? 0.5 : cfg.conf_thresh, p);
    Cam cam;
    cam.tag = SNCAL_CAM_NONE;
    const int st = ov_combine(mask, p, fp[frame].hs, fp[frame].hom, fp[frame].cs, fp[frame].cal, cam);
    if (lane != 0) return;
    if (defer_voter && st != ST_OK) {        // iterative_voter, prediction.py:245-257: left for the voter stage
        store_camera(out + frame, ST_NONE, cam);
        out[frame].status = STATUS_PENDING;
    } else {
        store_camera(out + frame, st, cam);
    }
}

// stand-alone Camera.refine_camera / Camera.solve_pnp on caller-provided 3-D / 2-D matches
__global__ __launch_bounds__(64) void pnp_kernel(const double* __restrict__ Kin, const double* __restrict__ p3,
                                                 const double* __restrict__ p2, const int* __restrict__ npts, int N,
                                                 double* __restrict__ rt, double* __restrict__ rmse, int mode,
                                                 int max_iters, double eps, int sched) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int n = min(npts[b], min(N, 64));
    const bool in = lane < n;
    double X[3] = {0, 0, 0}, u = 0, v = 0;
    if (in) {
        const double* q = p3 + ((size_t)b * N + lane) * 3;
        X[0] = q[0]; X[1] = q[1]; X[2] = q[2];
        u = p2[((size_t)b * N + lane) * 2]; v = p2[((size_t)b * N + lane) * 2 + 1];
    }
    const u64 mask = n >= 64 ? ~0ull : ((1ull << n) - 1);
    const K4 k{Kin[b * 4 + 0], Kin[b * 4 + 1], Kin[b * 4 + 2], Kin[b * 4 + 3]};
    double R[9], t[3], pos[3];
    for (int i = 0; i < 9; ++i) R[i] = rt[b * 12 + i];
    for (int i = 0; i < 3; ++i) pos[i] = rt[b * 12 + 9 + i];
    bool ok = true;
    if (mode == 0) {
        for (int i = 0; i < 3; ++i) t[i] = -(R[i * 3] * pos[0] + R[i * 3 + 1] * pos[1] + R[i * 3 + 2] * pos[2]);
        if (sched == SCHED_OPENCV) lm_solver_pose_auto(mask, R, t, k, X, u, v, max_iters, eps);
        else refine_pose_lm(mask, R, t, k, X, u, v, max_iters, eps);
    } else {
        // plane membership for the minimal solver = points with z == 0 (ids outside top_gates)
        const u64 gm = __ballot(in && X[2] == 0.0);
        ok = pnp_ransac(sched, mask, gm, k, X, u, v, R, t);
    }
    if (lane == 0 && ok) {
        for (int i = 0; i < 9; ++i) rt[b * 12 + i] = R[i];
        rt[b * 12 + 9] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
        rt[b * 12 + 10] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
        rt[b * 12 + 11] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    }
    if (rmse) {
        double z;
        const double e2 = reproj_e2(R, t, k, X, u, v, &z);
        const double m = wsum(in ? sqrt(e2) : 0.0) / (double)(n > 0 ? n : 1);
        if (lane == 0) rmse[b] = ok ? m : -1.0;
    }
}

// ---- host: pitch template upload ----------------------------------------------------------------------
void tangent_points(const double* c, double r, const double* p, double* a, double* b) {   // ellipse.py:20-33
    const double hyp = std::sqrt((p[0] - c[0]) * (p[0] - c[0]) + (p[1] - c[1]) * (p[1] - c[1]));
    const double th = std::acos(r / hyp), d = std::atan2(p[1] - c[1], p[0] - c[0]);
    a[0] = c[0] + r * std::cos(d + th); a[1] = c[1] + r * std::sin(d + th); a[2] = 0;
    b[0] = c[0] + r * std::cos(d - th); b[1] = c[1] + r * std::sin(d - th); b[2] = 0;
}

void build_pitch(double (*P)[3]) {   // soccerpitch.py:109-263 + ellipse.py:16-92, ids per ellipse.py:99-157
    const double hl = 52.5, hw = 34.0, PL = 16.5, PW = 40.32, GL = 5.5, GW = 18.32, PM = 11.0, Rr = 9.15, gy = 3.66, GH = 2.44;
    auto set = [&](int i, double x, double y, double z) { P[i][0] = x; P[i][1] = y; P[i][2] = z; };
    set(0, -hl, gy, -GH); set(1, -hl, -gy, -GH); set(2, -hl, gy, 0); set(3, -hl, -gy, 0);
    set(4, -hl + GL, GW / 2, 0); set(5, -hl + GL, -GW / 2, 0); set(6, -hl, GW / 2, 0); set(7, -hl, -GW / 2, 0);
    set(8, -hl + PL, PW / 2, 0); set(9, -hl + PL, -PW / 2, 0); set(10, -hl, PW / 2, 0); set(11, -hl, -PW / 2, 0);
    set(12, -hl, hw, 0); set(13, -hl, -hw, 0); set(14, 0, hw, 0); set(15, 0, -hw, 0);
    set(16, hl - PL, PW / 2, 0); set(17, hl - PL, -PW / 2, 0); set(18, hl, PW / 2, 0); set(19, hl, -PW / 2, 0);
    set(20, hl - GL, GW / 2, 0); set(21, hl - GL, -GW / 2, 0); set(22, hl, GW / 2, 0); set(23, hl, -GW / 2, 0);
    set(24, hl, -gy, -GH); set(25, hl, gy, -GH); set(26, hl, -gy, 0); set(27, hl, gy, 0);
    set(28, hl, hw, 0); set(29, hl, -hw, 0);
    const double c0[2] = {0, 0};
    double a[3], b[3];
    tangent_points(c0, Rr, P[15], a, b);
    set(30, a[0], a[1], 0); set(31, b[0], b[1], 0);
    tangent_points(c0, Rr, P[14], a, b);
    set(32, b[0], b[1], 0); set(33, a[0], a[1], 0);
    const double s = std::sqrt(2.0) * Rr / 2;
    set(34, s, -s, 0); set(35, -s, -s, 0); set(36, s, s, 0); set(37, -s, s, 0);
    set(38, Rr, 0, 0); set(39, -Rr, 0, 0); set(40, 0, -Rr, 0); set(41, 0, Rr, 0); set(42, 0, 0, 0);
    const double lpm[2] = {-hl + PM, 0}, rpm[2] = {hl - PM, 0};
    const double dx = PL - PM, ay = std::sqrt(Rr * Rr - dx * dx);
    set(43, lpm[0] + Rr, 0, 0); set(44, -hl + PL, ay, 0); set(45, -hl + PL, -ay, 0);
    tangent_points(lpm, Rr, P[9], a, b); set(46, a[0], a[1], 0);
    tangent_points(lpm, Rr, P[8], a, b); set(47, b[0], b[1], 0);
    set(48, lpm[0], 0, 0); set(49, P[8][0], 0, 0);
    set(50, rpm[0] - Rr, 0, 0); set(51, hl - PL, ay, 0); set(52, hl - PL, -ay, 0);
    tangent_points(rpm, Rr, P[17], a, b); set(53, b[0], b[1], 0);
    tangent_points(rpm, Rr, P[16], a, b); set(54, a[0], a[1], 0);
    set(55, rpm[0], 0, 0); set(56, P[16][0], 0, 0);
}

int ensure_pitch_uploaded() {
    static int rc = SNCAL_OK;
    // constant memory is per device: upload for the current device every time it changes
    static thread_local int last_dev = -1;
    int dev = 0;
    SNCAL_CHECK_HIP(hipGetDevice(&dev));
    if (dev == last_dev) return rc;
    double P[NPTS][3], P32[NPTS][3];
    build_pitch(P);
    for (int i = 0; i < NPTS; ++i)
        for (int j = 0; j < 3; ++j) P32[i][j] = (double)(float)P[i][j];
    SNCAL_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_P64), P, sizeof(P)));
    SNCAL_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(c_P32), P32, sizeof(P32)));
    last_dev = dev;
    return SNCAL_OK;
}

}  // namespace

// Scratch of the first pass (B x FirstPass) and of the voter's task stage (B x thresholds x VoterShared, ~0.8 KB each): one buffer per (device, stream),
// grown on demand and kept for the life of the process.  Calls on one stream are ordered, so the buffer is free again when the next
// call on that stream reaches its task stage.  Rounds 3-4 took it from hipMallocAsync / hipFreeAsync per call: with the solves of
// several batches on several streams (pipeline.py, round 5) an allocation that wants to reuse a block freed on ANOTHER stream made
// the HOST wait for that stream's solve -- the next forward was enqueued 164 ms late, measured (tools/dev/trace_queues.py).
namespace {
struct ScratchBuf { void* p = nullptr; size_t bytes = 0; };
std::mutex g_scratch_mu;
std::map<std::pair<int, hipStream_t>, ScratchBuf> g_scratch;
}
static int voter_scratch(hipStream_t st, size_t bytes, void** out) {
    int dev = 0;
    SNCAL_CHECK_HIP(hipGetDevice(&dev));
    void* old = nullptr;
    {   std::lock_guard<std::mutex> lock(g_scratch_mu);
        ScratchBuf& b = g_scratch[{dev, st}];
        if (b.bytes >= bytes) { *out = b.p; return SNCAL_OK; }
        old = b.p;                      // growth: the entry is taken out under the lock, the wait for the stream's solves happens outside it
        b.p = nullptr; b.bytes = 0;
    }
    if (old) { SNCAL_CHECK_HIP(hipStreamSynchronize(st)); (void)hipFree(old); }
    const size_t want = std::max(bytes, (size_t)1 << 20);
    void* p = nullptr;
    SNCAL_CHECK_HIP(hipMalloc(&p, want));
    {   std::lock_guard<std::mutex> lock(g_scratch_mu);
        ScratchBuf& b = g_scratch[{dev, st}];
        if (b.p) {                      // another thread grew the same (device, stream) entry meanwhile: keep the larger block
            if (b.bytes >= want) { (void)hipFree(p); *out = b.p; return SNCAL_OK; }
            void* q = b.p; b.p = nullptr;
            (void)hipStreamSynchronize(st); (void)hipFree(q);
        }
        b.p = p; b.bytes = want;
    }
    *out = p;
    return SNCAL_OK;
}

namespace sncal {
// sncal_stream_destroy / sncal_shutdown: the convenience form of sncal_calibrate keeps one scratch block per (device, stream); a stream
// that is destroyed takes its block with it (a later stream at the same address must not inherit a block the old stream's kernels may
// still be using: the release synchronises the stream first).  st == nullptr with all == true: every block of every device.
int release_solve_scratch(hipStream_t st, bool all) {
    std::vector<std::pair<std::pair<int, hipStream_t>, void*>> victims;
    {   std::lock_guard<std::mutex> lock(g_scratch_mu);
        for (auto it = g_scratch.begin(); it != g_scratch.end();) {
            if (all || it->first.second == st) { if (it->second.p) victims.push_back({it->first, it->second.p}); it = g_scratch.erase(it); }
            else ++it;
        }
    }
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& v : victims) {
        (void)hipSetDevice(v.first.first);
        (void)hipStreamSynchronize(v.first.second);
        (void)hipFree(v.second);
    }
    (void)hipSetDevice(cur);
    return SNCAL_OK;
}
}  // namespace sncal

static size_t calibrate_fp_bytes(int B) { return ((size_t)B * sizeof(FirstPass) + 255) & ~(size_t)255; }
static size_t calibrate_ws_bytes(int B, const sncal_voter_cfg* cfg) {
    return calibrate_fp_bytes(B) + (size_t)B * std::max(cfg->n_conf_threshs, 1) * sizeof(VoterShared);
}

extern "C" int sncal_calibrate_workspace(int B, const sncal_voter_cfg* cfg, size_t* bytes) {
    SNCAL_CHECK_ARG(B >= 0 && cfg && bytes, "sncal_calibrate_workspace: bad arguments");
    SNCAL_CHECK_ARG(cfg->n_conf_threshs >= 0 && cfg->n_conf_threshs <= SNCAL_MAX_CONF_THRESHS, "sncal_calibrate_workspace: n_conf_threshs");
    *bytes = std::max(calibrate_ws_bytes(B, cfg), (size_t)256);
    return SNCAL_OK;
}

static int calibrate_impl(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                          sncal_camera* d_out, void* d_ws, size_t ws_bytes, bool own_ws, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && cfg, "sncal_calibrate: bad arguments");
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_kpts && d_out, "sncal_calibrate: null pointer");
    SNCAL_CHECK_ARG(cfg->algorithm >= 0 && cfg->algorithm <= 4, "sncal_calibrate: algorithm %d", cfg->algorithm);
    SNCAL_CHECK_ARG(cfg->n_conf_threshs >= 0 && cfg->n_conf_threshs <= SNCAL_MAX_CONF_THRESHS, "sncal_calibrate: n_conf_threshs");
    SNCAL_CHECK_ARG(cfg->img_w > 1 && cfg->img_h > 1, "sncal_calibrate: image size");
    const int rc = ensure_pitch_uploaded();
    if (rc) return rc;
    // iterative_voter: frames whose first pass (original_voter) fails fall through to the voter at up to three thresholds,
    // 4x the work of the common case; in one kernel they were stragglers that set its duration (8.5 ms for 64 frames of
    // which 61 were done after 2.7 ms).  They are finished by a second launch that spreads the voter over four waves.
    const int defer = (cfg->algorithm == 0 && cfg->n_conf_threshs > 0) ? 1 : 0;
    hipStream_t st = sncal::as_stream(stream);
    // Every workgroup of the default path is ONE wavefront (first_pass_task_kernel above says why); SNCAL_SOLVE_WAVE_WGS=0 (tuning
    // aid / A-B reference, also what the byte-identity test compares with): round 4's paired 256-thread calibrate_kernel
    const bool wave_wgs = sncal::env_flag(sncal::ENV_SOLVE_WAVE_WGS);
    const bool paired = cfg->algorithm <= 1;
    // scratch: the first pass's per-frame slots, then the voter's per-(frame, threshold) slots -- the caller's workspace
    // (sncal_calibrate_ws) or the stream's own block (sncal_calibrate)
    const size_t fp_bytes = calibrate_fp_bytes(B);
    char* scratch = reinterpret_cast<char*>(d_ws);
    if (own_ws) {
        const int rcs = voter_scratch(st, calibrate_ws_bytes(B, cfg), reinterpret_cast<void**>(&scratch));
        if (rcs) return rcs;
    } else {
        SNCAL_CHECK_ARG(d_ws && (reinterpret_cast<uintptr_t>(d_ws) & 15) == 0, "sncal_calibrate_ws: workspace pointer (16-byte aligned device memory)");
        if (ws_bytes < calibrate_ws_bytes(B, cfg)) { sncal::set_error("sncal_calibrate_ws: workspace of %zu bytes, %zu needed (sncal_calibrate_workspace)", ws_bytes, calibrate_ws_bytes(B, cfg)); return SNCAL_ERR_WORKSPACE; }
    }
    if (paired && wave_wgs && (cfg->algorithm == 1 || defer)) {
        FirstPass* fp = reinterpret_cast<FirstPass*>(scratch);
        hipLaunchKernelGGL(first_pass_task_kernel, dim3((unsigned)(2 * B)), dim3(64), 0, st, d_kpts, d_line_pts, B, *cfg, fp);
        SNCAL_CHECK_LAUNCH();
        hipLaunchKernelGGL(first_pass_combine_kernel, dim3((unsigned)B), dim3(64), 0, st, d_kpts, d_line_pts, B, *cfg, (const FirstPass*)fp, d_out, defer);
        SNCAL_CHECK_LAUNCH();
    } else if (paired) {
        hipLaunchKernelGGL(calibrate_kernel, dim3((unsigned)((B + 1) / 2)), dim3(256), 0, st, d_kpts, d_line_pts, B, *cfg, d_out, defer);
        SNCAL_CHECK_LAUNCH();
    } else {                                 // voter / opencv_calibration(_multiplane): one wavefront per frame, no coupling between frames
        const int wpw = wave_wgs ? 1 : 4;
        hipLaunchKernelGGL(calibrate_kernel, dim3((unsigned)((B + wpw - 1) / wpw)), dim3(64 * wpw), 0, st, d_kpts, d_line_pts, B, *cfg, d_out, defer);
        SNCAL_CHECK_LAUNCH();
    }
    if (defer) {
        // one wavefront per (frame, threshold, camera) of the pending frames, then the selection in the reference's order.
        // SNCAL_SOLVE_TASKS=0 (tuning aid / A-B reference): the four-wave voter_kernel, thresholds one after the other
        if (sncal::env_flag(sncal::ENV_SOLVE_TASKS)) {
            VoterShared* slots = reinterpret_cast<VoterShared*>(scratch + fp_bytes);
            hipLaunchKernelGGL(voter_task_kernel, dim3((unsigned)(B * cfg->n_conf_threshs * VT_TASKS)), dim3(64), 0, st, d_kpts, d_line_pts, B, *cfg,
                               (const sncal_camera*)d_out, slots);
            SNCAL_CHECK_LAUNCH();
            hipLaunchKernelGGL(voter_select_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, *cfg, (const VoterShared*)slots, d_out);
            SNCAL_CHECK_LAUNCH();
        } else {
            hipLaunchKernelGGL(voter_kernel, dim3(B), dim3(256), 0, st, d_kpts, d_line_pts, B, *cfg, d_out);
            SNCAL_CHECK_LAUNCH();
        }
    }
    return SNCAL_OK;
}

extern "C" int sncal_calibrate(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                               sncal_camera* d_out, void* stream) {
    return calibrate_impl(d_kpts, d_line_pts, B, cfg, d_out, nullptr, 0, true, stream);
}

extern "C" int sncal_calibrate_ws(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                                  sncal_camera* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    return calibrate_impl(d_kpts, d_line_pts, B, cfg, d_out, d_ws, ws_bytes, false, stream);
}

// ---- sncal_calibrate_sweep --------------------------------------------------------------------------------------------------------------
// workspace: [FirstPass x B][VoterShared x B x T][sncal_camera x B: the first pass's result][SweepCand x B x T], each part on 256 bytes
namespace {
constexpr int SWEEP_MAX_GRID = 4096;
struct SweepLayout { int T; size_t slots, first, cands, bytes; };
size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }
SweepLayout sweep_layout(int B, const sncal_voter_cfg* cfg) {
    SweepLayout l;
    l.T = cfg->algorithm == 2 ? 1 : cfg->n_conf_threshs;
    l.slots = calibrate_fp_bytes(B);
    l.first = l.slots + up256((size_t)B * std::max(l.T, 1) * sizeof(VoterShared));
    l.cands = l.first + up256((size_t)B * sizeof(sncal_camera));
    l.bytes = std::max(l.cands + up256((size_t)B * std::max(l.T, 1) * sizeof(SweepCand)), (size_t)256);
    return l;
}
int sweep_check(const char* fn, int B, const sncal_voter_cfg* cfg, int n_grid) {
    SNCAL_CHECK_ARG(B >= 0 && cfg, "%s: bad arguments", fn);
    SNCAL_CHECK_ARG(cfg->algorithm >= 0 && cfg->algorithm <= 4, "%s: algorithm %d", fn, cfg->algorithm);
    SNCAL_CHECK_ARG(cfg->algorithm == 0 || cfg->algorithm == 2,
                    "%s: algorithm %d never reads max_rmse / max_rmse_rel, there is nothing to sweep (iterative_voter = 0 and voter = 2 do)", fn, cfg->algorithm);
    SNCAL_CHECK_ARG(cfg->n_conf_threshs >= 0 && cfg->n_conf_threshs <= SNCAL_MAX_CONF_THRESHS, "%s: n_conf_threshs", fn);
    SNCAL_CHECK_ARG(n_grid >= 1 && n_grid <= SWEEP_MAX_GRID, "%s: n_grid %d outside 1..%d", fn, n_grid, SWEEP_MAX_GRID);
    return SNCAL_OK;
}
}  // namespace

extern "C" int sncal_calibrate_sweep_workspace(int B, const sncal_voter_cfg* cfg, int n_grid, size_t* bytes) {
    const int rc = sweep_check("sncal_calibrate_sweep_workspace", B, cfg, n_grid);
    if (rc) return rc;
    SNCAL_CHECK_ARG(bytes, "sncal_calibrate_sweep_workspace: bad arguments");
    *bytes = sweep_layout(B, cfg).bytes;
    return SNCAL_OK;
}

extern "C" int sncal_calibrate_sweep(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg, const double* d_grid, int n_grid,
                                     sncal_camera* d_outcomes, int32_t* d_choice, void* d_ws, size_t ws_bytes, void* stream) {
    const int rca = sweep_check("sncal_calibrate_sweep", B, cfg, n_grid);
    if (rca) return rca;
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_kpts && d_grid && d_outcomes && d_choice, "sncal_calibrate_sweep: null pointer");
    SNCAL_CHECK_ARG(cfg->img_w > 1 && cfg->img_h > 1, "sncal_calibrate_sweep: image size");
    SNCAL_CHECK_ARG(d_ws && (reinterpret_cast<uintptr_t>(d_ws) & 15) == 0, "sncal_calibrate_sweep: workspace pointer (16-byte aligned device memory)");
    const SweepLayout lay = sweep_layout(B, cfg);
    if (ws_bytes < lay.bytes) { sncal::set_error("sncal_calibrate_sweep: workspace of %zu bytes, %zu needed (sncal_calibrate_sweep_workspace)", ws_bytes, lay.bytes); return SNCAL_ERR_WORKSPACE; }
    const int rc = ensure_pitch_uploaded();
    if (rc) return rc;
    hipStream_t st = sncal::as_stream(stream);
    char* const ws = reinterpret_cast<char*>(d_ws);
    FirstPass* const fp = reinterpret_cast<FirstPass*>(ws);
    VoterShared* const slots = reinterpret_cast<VoterShared*>(ws + lay.slots);
    sncal_camera* const first = reinterpret_cast<sncal_camera*>(ws + lay.first);
    SweepCand* const cands = reinterpret_cast<SweepCand*>(ws + lay.cands);
    const int T = lay.T;
    sncal_voter_cfg c = *cfg;                    // what the solve kernels see: the thresholds as the task stage indexes them
    if (cfg->algorithm == 2) {
        c.n_conf_threshs = 1; c.conf_threshs[0] = cfg->conf_thresh;
        hipLaunchKernelGGL(sweep_mark_pending_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, B, first);
        SNCAL_CHECK_LAUNCH();
    } else {                                     // the stages of sncal_calibrate's default path, unchanged
        hipLaunchKernelGGL(first_pass_task_kernel, dim3((unsigned)(2 * B)), dim3(64), 0, st, d_kpts, d_line_pts, B, c, fp);
        SNCAL_CHECK_LAUNCH();
        hipLaunchKernelGGL(first_pass_combine_kernel, dim3((unsigned)B), dim3(64), 0, st, d_kpts, d_line_pts, B, c, (const FirstPass*)fp, first, T > 0 ? 1 : 0);
        SNCAL_CHECK_LAUNCH();
    }
    if (T > 0) {
        hipLaunchKernelGGL(voter_task_kernel, dim3((unsigned)(B * T * VT_TASKS)), dim3(64), 0, st, d_kpts, d_line_pts, B, c, (const sncal_camera*)first, slots);
        SNCAL_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sweep_outcomes_kernel, dim3((unsigned)((B * (T + 1) + 63) / 64)), dim3(64), 0, st, B, T, (const sncal_camera*)first,
                       (const VoterShared*)slots, d_outcomes, cands);
    SNCAL_CHECK_LAUNCH();
    const size_t n = (size_t)n_grid * B;
    hipLaunchKernelGGL(sweep_select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B, T, n_grid, d_grid, (const sncal_camera*)first,
                       (const SweepCand*)cands, d_choice);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

static int env_schedule() {      // SNCAL_SOLVE_SCHEDULE=converged: the two single-camera entries on the run-to-convergence minimisers
    const char* v = sncal::env_str(sncal::ENV_SOLVE_SCHEDULE);
    return v && !strcmp(v, "converged") ? SCHED_CONVERGED : SCHED_OPENCV;
}

static int launch_pnp(const double* d_K, const double* d_pts3d, const double* d_pts2d, const int32_t* d_npts, int B, int N,
                      double* d_rt, double* d_rmse, int mode, int max_iters, double eps, void* stream) {
    SNCAL_CHECK_ARG(B >= 0 && N > 0 && N <= 64, "pnp: need 0 < N <= 64 points per frame (got %d)", N);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG(d_K && d_pts3d && d_pts2d && d_npts && d_rt, "pnp: null pointer");
    hipLaunchKernelGGL(pnp_kernel, dim3(B), dim3(64), 0, sncal::as_stream(stream), d_K, d_pts3d, d_pts2d, d_npts, N, d_rt,
                       d_rmse, mode, max_iters, eps, env_schedule());
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

extern "C" int sncal_pnp_refine_lm(const double* d_K, const double* d_pts3d, const double* d_pts2d, const int32_t* d_npts,
                                   int B, int N, double* d_rt, double* d_rmse, int max_iters, double eps, void* stream) {
    const bool cv = env_schedule() == SCHED_OPENCV;      // defaults = the criteria camera.py:116-117 passes: (20000, 1e-5)
    return launch_pnp(d_K, d_pts3d, d_pts2d, d_npts, B, N, d_rt, d_rmse, 0, max_iters > 0 ? max_iters : (cv ? 20000 : 100),
                      eps > 0 ? eps : (cv ? 1e-5 : 1e-10), stream);
}

extern "C" int sncal_solve_pnp(const double* d_K, const double* d_pts3d, const double* d_pts2d, const int32_t* d_npts,
                               int B, int N, double* d_rt, void* stream) {
    return launch_pnp(d_K, d_pts3d, d_pts2d, d_npts, B, N, d_rt, nullptr, 1, 20, 1e-10, stream);
}
