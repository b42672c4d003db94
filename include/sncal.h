/*
 * sncal.h -- C ABI of libsncal.so: the MI355X (gfx950) implementation of the per-frame camera
 * calibration hot path of NikolasEnt/soccernet-calibration-sportlight.
 *
 * The reference has no FFI: the path sits behind three Python call surfaces.  Each
 * entry point below names the reference interface it replaces (file:line under /root/reference);
 * the Python host mirror (the .py files of soccernet-calibration-sportlight_amd) binds them with ctypes and
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative sncal_status; the message of the last
 *     failure on the calling thread is available from sncal_last_error();
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); nothing synchronises
 *     the stream or the device unless stated;
 *   - pointers named d_* are DEVICE pointers, h_* are HOST pointers; the library never allocates
 *     behind the caller's back on the data path: scratch comes from caller-provided workspaces
 *     whose size is returned by the matching *_workspace() query (the one exception is the
 *     convenience form sncal_calibrate, documented there; sncal_calibrate_ws follows the rule);
 *   - no torch / C++ types cross the boundary: plain pointers, ints, floats, doubles.
 */
#ifndef SNCAL_H
#define SNCAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNCAL_VERSION 100

typedef enum {
    SNCAL_OK = 0,
    SNCAL_ERR_ARG = -1,        /* invalid argument (shape, null pointer, unsupported size)  */
    SNCAL_ERR_HIP = -2,        /* a HIP runtime call or kernel launch failed                */
    SNCAL_ERR_STATE = -3,      /* object not finalised / weights missing                    */
    SNCAL_ERR_WORKSPACE = -4,  /* caller workspace too small                                */
    SNCAL_ERR_UNSUPPORTED = -5,/* well-formed input that this build does not handle (e.g. progressive JPEG) */
    SNCAL_ERR_RANGE = -6       /* fp16x3 engine: a folded weight (finalize) or an activation (sncal_hrnet_range_status) outside what
                                  fp16 hi + lo halves represent; the reference's fp32 predict() has no such limit: use SNCAL_F32 */
} sncal_status;

typedef enum { SNCAL_F32 = 0, SNCAL_BF16 = 1, SNCAL_FP8 = 2, SNCAL_BF16X3 = 3 } sncal_dtype;

int sncal_version(void);
const char* sncal_last_error(void);
/* Name of the split-arithmetic engine this library was built with (SNCAL_BF16X3): "fp16x3" (fp16 hi + fp16 lo, the default since round 4)
 * or "bf16x3" (bf16 hi + lo, -DSNCAL_X3_F16=0).  No reference counterpart: the reference's predict() is plain fp32
 * (src/models/hrnet/metamodel.py:127-134); the engine reproduces it on the 16-bit matrix pipe (NOTES/design_history_r1_r5.md §9.3 / 10). */
const char* sncal_x3_name(void);

/* ------------------------------------------------------------------------------------------------
 * D1  keypoint heatmap decode
 * replaces HRNetPredictionTransform.__call__  src/models/hrnet/transforms.py:228-239
 *   d_logp  (B,C,h,w) fp32 log-probabilities, NCHW contiguous
 *   d_out   (B,C-1,3) fp32 rows [x_px, y_px, conf]; the last (background) channel is dropped
 *   x = first column holding the channel maximum of exp(logp), y = first row holding it (the two
 *   come from separate reductions, exactly like the reference), conf = that maximum,
 *   x_px = x*img_w/w, y_px = y*img_h/h.   exp is float32(exp(float64(.))) -- see oracle/decode.py.
 *   Size limit: h <= 8192, w <= 2048 and (h + 5*w + 4) * 4 <= 65536 bytes -- one workgroup keeps a plane's row and
 *   column maxima in 64 KiB of LDS (6140 x 2048 and 8192 x 1637 are the largest at either end); anything larger is
 *   SNCAL_ERR_ARG, and the message names the shape and the bound.
 * ---------------------------------------------------------------------------------------------- */
int sncal_heatmap_decode(const float* d_logp, int B, int C, int h, int w, int img_h, int img_w,
                         float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L2  line heatmap 2-peak decode
 * replaces EHMPredictionTransform.__call__ / mask_heat_points_gauss
 *          src/models/line/transforms.py:217-280
 *   d_heat (B,C,h,w) fp32;  d_out (B,C,2,3) fp32 rows [x*scale, y*scale, value]
 * ---------------------------------------------------------------------------------------------- */
int sncal_line_decode(const float* d_heat, int B, int C, int h, int w, float sigma, float scale,
                      float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * L3 + L4  line peaks -> line equations -> the 30 intersection keypoint candidates
 * replaces get_line_data / calculate_slope_intercept  src/utils/export_line_result.py:51-131,
 *          CameraCreator.__init__ lines ingestion     src/models/hrnet/prediction.py:105-124,
 *          line_eq_intersection                       src/models/hrnet/prediction.py:643-653
 *   d_peaks (B,23,2,3) fp32 rows [x, y, p] in heatmap units (sncal_line_decode with scale 1; LINE_CLS order);
 *   d_out   (B,30,3) fp32 rows [x, y, valid] = sncal_calibrate's d_line_pts (ids of LINE_INTERSECTIONS).
 * Arithmetic as in the reference's pinned numpy 1.24.2: float32 coordinates, float64 from `+ 1e-5` on.
 * ---------------------------------------------------------------------------------------------- */
int sncal_lines_to_points(const float* d_peaks, int B, float scale, double prob_thre, float* d_out,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * M1-M5, L1  HRNet keypoint / line network
 * replaces HighResolutionNet.__init__/forward  src/models/hrnet/hrnet.py:255-355, 437-511,
 *          src/models/line/hrnet.py:30-249, HRNetHeatmap.forward src/models/hrnet/model.py:143-150
 * The descriptor carries the fields of the reference's model_config yaml
 * (src/models/hrnet/model_config/hrnet_w48.yaml).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int num_classes;            /* 58 keypoint net, 23 line net                                  */
    int stem_width;             /* 64                                                            */
    int upscale;                /* head size / branch 0 size.  1: line net (branches only); 2, 4:   */
                                /* all branches AND the stem, bilinear, concatenated (hrnet_w48x4: 4) */
    int head_softmax;           /* 0 = LogSoftmax(dim=1) head, 1 = Softmax(dim=1) head           */
    int stage1_blocks;          /* number of Bottleneck blocks in layer1                         */
    int stage1_channels;        /* Bottleneck planes (output = 4x)                               */
    int num_modules[3];         /* stage2..4                                                     */
    int num_branches[3];        /* 2,3,4                                                         */
    int num_blocks[3];          /* BasicBlocks per branch (uniform per stage in every config)    */
    int num_channels[3][4];     /* branch widths per stage                                       */
} sncal_hrnet_desc;

typedef struct sncal_hrnet sncal_hrnet;

/* Build the execution plan (no weights yet).  dtype selects the arithmetic of the conv kernels:
 * SNCAL_BF16 = bf16 activations/weights with fp32 MFMA accumulation (fast path),
 * SNCAL_F32  = fp32 activations/weights on the exact-fp32 MFMA (parity path),
 * SNCAL_BF16X3 = the fp32 engine (fp32 activations, fp32 accumulation) with SPLIT-bf16 arithmetic in the 3x3 stride-1 convolutions of
 *              stages 2-4: x = hi + lo, w = hi + lo in bf16, hi.hi + hi.lo + lo.hi on the bf16 MFMA -- fp32-class results (|dlogp| ~ 5e-6
 *              against the exact engine, same keypoint indices) at a multiple of the fp32 MFMA rate,
 * SNCAL_FP8  = the bf16 engine with OCP e4m3 arithmetic (CDNA4 block-scaled MFMA, K = 64) in the wide 3x3 stride-1
 *              convolutions of stages 2-4 (BASELINE config 5); needs sncal_hrnet_calibrate_fp8 before the first forward. */
int sncal_hrnet_create(const sncal_hrnet_desc* desc, int dtype, sncal_hrnet** out);
void sncal_hrnet_destroy(sncal_hrnet* net);

/* The plan's conv units in the reference's registration order, with the state-dict prefixes the
 * host needs to fetch weights ("model.stage3.2.branches.1.0.conv1" / "...bn1"). */
int sncal_hrnet_num_convs(const sncal_hrnet* net);
int sncal_hrnet_conv_info(const sncal_hrnet* net, int idx, char* name, int name_cap, char* bn_name,
                          int bn_cap, int* cin, int* cout, int* ksize, int* stride, int* has_bias);
/* Give conv `idx` its weights: h_weight (Cout,Cin,k,k) fp32 host, h_scale/h_shift (Cout) fp32 host
 * = the eval-mode BatchNorm folded to y = conv(x)*scale + shift (scale NULL => 1). */
int sncal_hrnet_set_conv(sncal_hrnet* net, int idx, const float* h_weight, const float* h_scale,
                         const float* h_shift);
/* Pack + upload all weights (synchronous).  Every conv must have been set.
 * SNCAL_BF16X3 built with fp16 halves ("fp16x3", the default engine) carries every operand as fp16 hi + lo: exact to 2^-22 relative for
 * |v| in [2^-3, 65504], to 2^-25 absolute below, CLAMPED at +-65504 above.  The reference's predict() is plain fp32 with no such limits
 * (src/models/hrnet/metamodel.py:127-134), so the engine guards both ends of the clamp:
 *   here      SNCAL_ERR_RANGE when a folded weight (w * gamma / sqrt(var + eps)) exceeds 65504 in magnitude, is not finite, or when most of
 *             a layer's weight mass lies below 2^-14 (fp16's smallest normal: the halves keep fewer than 11 bits there); the message
 *             names the layer.  Callers fall back to SNCAL_F32 (the host mirror's load_model does so by itself, with a warning);
 *   forward   every kernel that splits activations counts the wavefronts that met |v| > 65504: sncal_hrnet_range_status below.
 *   balance   (fp16x3 only, default ON) before packing, finalize rebalances block-internal channels by exact powers of two: the tensor
 *             between conv1 and conv2 of a BasicBlock (conv1 / conv2, conv2 / conv3 of a Bottleneck; src/models/hrnet/hrnet.py:42-58, 79-99)
 *             has ONE consumer, so producer row c x 2^-l and consumer column c x 2^l is the same fp32 network bit for bit, and choosing l so
 *             that weight and activation are of one size keeps the fp16 halves at their full 22 bits on checkpoints whose BatchNorm scales
 *             spread over decades (csrc/hrnet.cpp equalize_blocks; only channels >= 2^4 away from an ordinary checkpoint's balance move).
 *             sncal_hrnet_set_equalize(net, 0) switches it off; sncal_hrnet_equalize runs the same step on its own (host only: no GPU
 *             needed) and reports the number of channels moved; sncal_hrnet_get_conv reads a conv's host parameters back (between
 *             sncal_hrnet_set_conv and sncal_hrnet_finalize, which releases them).  No reference counterpart (the reference is fp32).
 * A network handle is SINGLE-STREAM: forwards of one handle on two streams at once would share its work-ticket words. */
int sncal_hrnet_finalize(sncal_hrnet* net);
int sncal_hrnet_set_equalize(sncal_hrnet* net, int enable);
int sncal_hrnet_equalize(sncal_hrnet* net, int* moved);
int sncal_hrnet_get_conv(const sncal_hrnet* net, int idx, float* h_weight, float* h_scale, float* h_shift);
/* Range flag of the split-fp16 engine since the last clear: *overflow = wavefronts that split (and clamped) an activation beyond +-65504,
 * *nonfinite = workgroups of the input layout kernel that met a NaN / infinite frame value.  Returns SNCAL_OK when both are zero,
 * SNCAL_ERR_RANGE otherwise (sncal_last_error says what to do: such forwards are not the reference's fp32 result).  Synchronises
 * `stream`; clear != 0 re-arms the counters.  Engines without the clamp (SNCAL_F32, SNCAL_BF16, SNCAL_FP8, the bf16x3 build) report zeros.
 * No reference counterpart: the reference computes in fp32 (metamodel.py:127-134) and cannot overflow where this engine can. */
int sncal_hrnet_range_status(sncal_hrnet* net, unsigned* overflow, unsigned* nonfinite, int clear, void* stream);

/* Output spatial size and workspace bytes for a (B,3,H,W) input. */
int sncal_hrnet_output_size(const sncal_hrnet* net, int H, int W, int* out_h, int* out_w);
int sncal_hrnet_workspace(const sncal_hrnet* net, int B, int H, int W, size_t* bytes);

/* Forward.  d_x (B,3,H,W) fp32 NCHW in [0,1] (what make_submit.py:66-67 builds).
 *   d_heat  optional (B,num_classes,h,w) fp32 NCHW head output (log-softmax / softmax)
 *   d_kpts  optional (B,num_classes-1,3) fp32 decoded keypoints (keypoint net only; D1 semantics
 *           with size = (img_h,img_w))
 * At least one of d_heat / d_kpts must be non-NULL. */
int sncal_hrnet_forward(sncal_hrnet* net, const float* d_x, int B, int H, int W, float* d_heat,
                        float* d_kpts, int img_h, int img_w, void* d_ws, size_t ws_bytes,
                        void* stream);

/* C5 (BASELINE.json configs[4]: "HRNet-W48 fp8 (CDNA4 fp8 MFMA) 1920x1080 ... reproj-error tolerance sweep").  No reference
 * counterpart: HRNetMetaModel.predict is fp32 (src/models/hrnet/metamodel.py:127-134); the reference's AMP autocast exists
 * only in its train / val steps (:34, :67).
 * calibrate: one bf16 forward of d_x (B,3,H,W) that records max |x| of every tensor feeding an fp8-capable convolution
 *            (BasicBlock conv1 / conv2 of the 96 / 192 / 384-channel branches, src/models/hrnet/hrnet.py:42-58) ->
 *            per-tensor activation scales amax / 448; weights carry one scale per output channel.
 * set_fp8_layers: which of those convolutions run in fp8 -- "all", "none", or a comma list of stage2..stage4 and c<width>
 *            (a layer is selected when its stage AND its width are selected; an empty class selects all of it).  The
 *            tolerance sweep of tests/test_fp8_gpu.py walks this selection. */
int sncal_hrnet_calibrate_fp8(sncal_hrnet* net, const float* d_x, int B, int H, int W, void* d_ws, size_t ws_bytes, void* stream);
/* Workspace bytes of that calibration forward.  It runs every layer in bf16, without the e4m3 twins: on a network that is already
 * calibrated its layout is not the one sncal_hrnet_workspace describes, and may need MORE bytes.  NOT a pure query: it lays the network
 * out as the calibration would and then drops that layout, like sncal_hrnet_set_fp8_layers -- cached launch schedules and their device work
 * lists are freed, sncal_hrnet_plan_op / plan_tensor are invalid until the next sncal_hrnet_workspace or forward, which lay out again. */
int sncal_hrnet_calibrate_fp8_workspace(sncal_hrnet* net, int B, int H, int W, size_t* bytes);
int sncal_hrnet_set_fp8_layers(sncal_hrnet* net, const char* spec);

/* Same forward from the frames as the reference's harness holds them BEFORE torchvision's ToTensor
 * (make_submit.py:62-66: cv2.imread -> BGR uint8 (H,W,3) -> ToTensor = float32 x/255, CHW): d_x (B,H,W,3) uint8.
 * Bit-identical to sncal_hrnet_forward on ToTensor's output; the input read is 3 bytes per pixel instead of 12
 * (at thousands of frames per second the float frames are the PCIe / HBM bottleneck). */
int sncal_hrnet_forward_u8(sncal_hrnet* net, const unsigned char* d_x, int B, int H, int W, float* d_heat,
                           float* d_kpts, int img_h, int img_w, void* d_ws, size_t ws_bytes,
                           void* stream);

/* Diagnostics (measurement only, no reference counterpart): per-kernel timing of forwards with HIP events
 * recorded on the caller's stream between the plan's launches.  Enable, run forwards, then read the
 * accumulated per-kernel-variant totals (the call synchronises the recorded events). */
typedef struct {
    char kernel[96];        /* e.g. "conv<bf16,k3,s1,NI4,MI6,G4>", "upsample_add", "softmax_nchw", "kp_decode" */
    double flops;           /* algorithmic FLOPs (2*MACs of the direct formulation) summed over launches  */
    double bytes;           /* algorithmic HBM bytes (inputs read once + outputs written once) summed     */
    double ms;              /* summed event-to-event time                                                */
    int launches;
} sncal_kernel_stat;
/* enable: 0 off; 1 time every launch; 2 time only the launches of the kernel variant that led the profile recorded so
 * far (needs a preceding mode-1 profile; the timing events cost ~4 us per launch, so a timed region that only needs
 * its dominant kernel's duration should not pay for the other ~150 launches). Every call clears the recorded profile. */
int sncal_hrnet_set_profiling(sncal_hrnet* net, int enable);
int sncal_hrnet_get_profile(sncal_hrnet* net, sncal_kernel_stat* out, int cap, int* count);

/* Plan introspection + taps (test instrumentation, no reference counterpart): the per-kernel parity tests
 * (tests/test_kernels_gpu.py) check EVERY launch of a forward -- each convolution of src/models/hrnet/hrnet.py:42-58, 79-99,
 * 183-246, 357-391, the fuse sums of :229-244, the head of :316-329, 489-510 -- against torch fp32 on the operands that launch
 * really read.  The plan is the flat op list the executor walks; tensors are NHWC slots of the caller's workspace.  A tap
 * copies one tensor of the FIRST sub-batch into a caller buffer (device-to-device, on the forward's stream) when the
 * executor passes the given op -- after the launch that ran it, also when that launch was a grouped / fused one issued at
 * an earlier op -- while the tensor is still alive.  Taps never change what is launched. */
typedef struct {
    int type;                  /* 0 input layout, 1 conv, 2 upsample_add, 3 softmax, 4 decode, 5 fused head                    */
    int active;                /* part of the plan at the current layout (three head formulations live side by side)         */
    int conv;                  /* conv unit (index as in sncal_hrnet_conv_info; >= num_convs: head-internal slice of last_layer.0) */
    char name[96];             /* its name, "" for non-conv ops                                                                */
    int cin, cout, ksize, stride, col_off;   /* col_off: first column of last_layer.0 of a head-internal slice               */
    int in, res, out, base;    /* tensor ids (-1 = none)                                                                       */
    int src[4], nsrc;          /* upsample_add sources                                                                         */
    int head_direct, head_src[5], head_nsrc, head_fold[3], head_nfold;   /* head_direct -1: no tensor sits at head resolution
                                  (upscale 4); the stem then leads head_fold                                                   */
    int relu, out_coff, out_f32, fp8;        /* fp8: 1 = this conv runs in e4m3 at the current layout, 2 = in split bf16 on the two-team kernel (bf16x3), 3 = in split bf16 on the generic kernel */
    char kernel[96];           /* label of the launch that executed it in the last mode-1 profiled forward ("" = unknown or
                                  executed by the launch of an earlier op: grouped members, second conv of a fused block)      */
    int res_twin;              /* bf16x3: this conv reads its residual from the split twin of tensor `res`, not from its fp32 form */
    int launch;                /* index, in the launch schedule of the layout's own sub-batch size, of the launch that covers this op
                                  (grouped members and the ops of a fused pair share one); -1 = inactive or no schedule yet        */
    /* What that schedule decided for the op (all 0 when inactive or no schedule yet): */
    int writes_out;            /* 1 = the launch covering this op writes tensor `out` in its dense form (0 for the first op of a fused
                                  pair whose output stays in LDS, and for a producer whose dense form nobody reads)                 */
    int writes_twin;           /* 1 = that launch writes the e4m3 / split twin of `out`                                            */
    int prep_in;               /* the helper in front of the launch that makes the twin of `in`: 0 none, 1 quantize_fp8, 2 split_f32 */
} sncal_plan_op;
typedef struct {
    int C, H, W;               /* NHWC, per frame                                                                              */
    int dtype;                 /* 0 fp32, 1 bf16, 2 e4m3                                                                       */
    int twin;                  /* id of the tensor's e4m3 twin or -1                                                           */
    int alive;                 /* allocated at the current layout                                                              */
    float scale;               /* e4m3 twins: value = code * scale                                                             */
    size_t bytes;              /* of the first sub-batch (sub_batch frames)                                                    */
    int sub_batch;
    size_t offset;             /* byte offset of the slot in the workspace (alive tensors)                                     */
    int first, last;           /* ops between which the allocator keeps the slot (lifetimes as stretched over launch groups and
                                  fusable pairs), -1 = not allocated                                                           */
} sncal_plan_tensor;
int sncal_hrnet_plan_num_ops(const sncal_hrnet* net);
int sncal_hrnet_plan_num_tensors(const sncal_hrnet* net);
/* Valid after sncal_hrnet_workspace / a forward at the shape of interest (the layout decides sizes, twins and head variant);
 * on a finalized network sncal_hrnet_workspace also builds the launch schedule of that sub-batch size (host work only), so that
 * sncal_plan_op.launch, writes_out, writes_twin and prep_in are valid without a forward. */
int sncal_hrnet_plan_op(const sncal_hrnet* net, int idx, sncal_plan_op* out);
int sncal_hrnet_plan_tensor(const sncal_hrnet* net, int id, sncal_plan_tensor* out);
/* Register a tap (op_idx >= 0) or clear all taps (op_idx < 0).  d_dst must hold sncal_plan_tensor.bytes. */
int sncal_hrnet_plan_tap(sncal_hrnet* net, int op_idx, int tensor_id, void* d_dst);

/* ------------------------------------------------------------------------------------------------
 * S0-S11  camera solve (batched, one wavefront per frame)
 *         sncal_calibrate / _ws: one configuration; sncal_calibrate_sweep: the same solve, every (max_rmse, max_rmse_rel) of a grid
 * ---------------------------------------------------------------------------------------------- */
typedef struct {              /* one solved camera; mirrors baseline/camera.py:79-90 attributes     */
    double position[3];
    double rotation[9];       /* row-major R, X_cam = R (X_world - position)                       */
    double fx, fy;            /* calibration[0,0], calibration[1,1]                                */
    double cx, cy;            /* calibration[0,2], [1,2] used by solve_pnp/refine (Q3)             */
    double rmse;              /* Camera.projection_rmse of the selected camera (mean L2, px)       */
    int32_t status;           /* 0 = no camera (reference returns None), >0 = which branch produced it */
    int32_t n_points;         /* size of the matched-point set `rmse` is the mean over: the selection plus the admitted line
                                 points (status 1, 2, 5, 7; opencv_calibration: its ground points), that set cut to keep_points
                                 (3) / to the ground plane (6), the H-consistent ground points plus the top gates (4); 0 with status 0 */
} sncal_camera;

enum {                        /* sncal_camera.status                                               */
    SNCAL_CAM_NONE = 0,
    SNCAL_CAM_ORIGINAL = 1,       /* original_voter calibrate path  prediction.py:396-433          */
    SNCAL_CAM_ORIGINAL_HOM = 2,   /* original_voter homography fallback  :434-436                  */
    SNCAL_CAM_VOTER_REL = 3, SNCAL_CAM_VOTER_ACC = 4, SNCAL_CAM_VOTER_ALL = 5,
    SNCAL_CAM_VOTER_GROUND = 6,   /* voter winners  :293-323                                       */
    SNCAL_CAM_VOTER_HOM = 7       /* voter homography fallback  :327-329                           */
};

#define SNCAL_MAX_CONF_THRESHS 16   /* the reference loops over any number of thresholds (prediction.py:245-257); make_submit.py passes 3 */
typedef struct {              /* CameraCreator kwargs, make_submit.py:45-50                        */
    int algorithm;            /* 0 iterative_voter, 1 original_voter, 2 voter,
                                 3 opencv_calibration, 4 opencv_calibration_multiplane            */
    int n_conf_threshs;
    double conf_thresh;       /* compared in double, like numpy's float32-scalar > python-float      */
    double conf_threshs[SNCAL_MAX_CONF_THRESHS];   /* iterative_voter's thresholds in the order they are tried; the first n_conf_threshs count */
    double max_rmse, max_rmse_rel;
    int min_points, min_points_per_plane, min_points_for_refinement, reliable_thresh;
    double min_focal_length;
    int img_w, img_h;
    int lm_schedule;          /* 0 (default) = the minimisers follow OpenCV 4.7's own schedules as far as they are known:
                                 LMSolver for solvePnPRefineLM (lambda_0 = 1, D fixed, gain ratio, stop 1e-5), CvLevMarq for the
                                 extrinsics refits (20 iterations / FLT_EPSILON) and calibrateCamera's joint fit (30 / DBL_EPSILON);
                                 1 = run every minimiser to convergence (the build's round-1/2 specification).  OpenCV parity is
                                 unpinned either way (cv2 is not installable offline).  ABI note: 0 became the OpenCV schedules in
                                 round 3 -- a caller that zero-initialises this struct gets them; set 1 for the round-1/2 behaviour */
    int refine_max_iters;     /* iteration cap of Camera.refine_camera's LM under lm_schedule 0; 0 = 20000 = what the reference passes
                                 (camera.py:116; rounds 1-3 defaulted to 200).  Well-posed frames stop on the 1e-5 step test within
                                 ~25 iterations; the runs that used to need the cap were voter candidates calibrated to f ~ 0.04 px,
                                 which good_camera discards whatever their pose: those are no longer refined at all              */
} sncal_voter_cfg;

/* Camera.refine_camera  baseline/camera.py:105-119 (cv.solvePnPRefineLM, K fixed, 6-DoF pose LM; LMSolver's schedule, see
 * sncal_voter_cfg.lm_schedule; max_iters <= 0 / eps <= 0 select the reference's (20000, 1e-5), see sncal_voter_cfg.refine_max_iters; the environment variable
 * SNCAL_SOLVE_SCHEDULE=converged switches this entry and sncal_solve_pnp to the run-to-convergence minimisers).
 *   d_K (B,4) fx,fy,cx,cy   d_pts3d (B,N,3) fp64   d_pts2d (B,N,2) fp64   d_npts (B) int32
 *   d_rt (B,12) in/out: rotation row-major (9) + position (3)   d_rmse (B) out mean-L2 px */
int sncal_pnp_refine_lm(const double* d_K, const double* d_pts3d, const double* d_pts2d,
                        const int32_t* d_npts, int B, int N, double* d_rt, double* d_rmse,
                        int max_iters, double eps, void* stream);

/* Camera.solve_pnp  baseline/camera.py:92-103 (cv.solvePnPRansac + Rodrigues), same layouts. */
int sncal_solve_pnp(const double* d_K, const double* d_pts3d, const double* d_pts2d,
                    const int32_t* d_npts, int B, int N, double* d_rt, void* stream);

/* CameraCreator.__call__  src/models/hrnet/prediction.py:130-136 with every algorithm of :90-96.
 *   d_kpts (B,57,3) fp32 decoded keypoints   d_line_pts (B,30,3) fp32 [x,y,valid] or NULL
 *   d_out (B) sncal_camera.  Never fails per frame: status 0 == the reference's `None`.
 * Asynchronous on `stream`.  iterative_voter runs as stages on that stream: the original_voter pass (one wavefront per frame and half:
 * its homography camera and its calibrated camera), then, for the frames it left without a camera, one wavefront per threshold x voter
 * camera and a selection in the reference's threshold order (prediction.py:250-256).
 * Scratch (per-frame slots of the two stages):
 *   sncal_calibrate_ws   the library's convention: the caller provides d_ws of at least sncal_calibrate_workspace(B, cfg) bytes
 *                        (16-byte aligned device memory, free to reuse once the work enqueued on `stream` has passed it); nothing
 *                        persists between calls.  The host mirror (CameraCreator.solve_device) uses this form.
 *   sncal_calibrate      convenience form without a workspace argument: the library keeps ONE scratch block per (device, stream),
 *                        hipMalloc'ed at the stream's first call, grown when a larger batch arrives, and reused by later calls on that
 *                        stream (stream order makes that safe; rounds 3-4 took it from hipMallocAsync per call, which made the HOST wait
 *                        for other streams' solves).  The block is released by sncal_stream_destroy(stream) for streams created here, and
 *                        by sncal_shutdown() for all streams -- call it before destroying a stream created elsewhere whose handle value
 *                        may be reused.
 * RANSAC sampling -- a KNOWN DEVIATION from the reference's numbers: cv2.findHomography (src/datatools/ellipse.py:497, used through
 * prediction.py:487-500) and cv.solvePnPRansac (baseline/camera.py:100-101) draw their minimal samples from OpenCV's fixed-seed RNG
 * (a multiply-with-carry generator); this library draws the four indices of hypothesis h from its own counter hash of (h, draw) --
 * the same 128 samples for every frame with the same point count, evaluated lane-parallel -- and takes the hypothesis with the most
 * inliers (ties: smaller squared error, then lower h) where OpenCV keeps the first best and adapts its iteration count.  Both are
 * deterministic and both refit on the winner's inliers, so on frames whose keypoints are all inliers of one model the refit -- hence the camera -- does not
 * depend on the draw; on frames with gross outliers a different draw may find a different inlier set and therefore a different camera
 * than OpenCV would.  Unmeasurable here (no cv2 on this image), stated so that nobody takes it for parity. */
int sncal_calibrate(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                    sncal_camera* d_out, void* stream);
int sncal_calibrate_workspace(int B, const sncal_voter_cfg* cfg, size_t* bytes);
int sncal_calibrate_ws(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                       sncal_camera* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* Free what the library holds outside its handles (the scratch blocks of sncal_calibrate above); synchronises those streams. */
int sncal_shutdown(void);

/* One solve, a whole grid of (max_rmse, max_rmse_rel) -- the two parameters optimize_valid.yaml tunes.  They are read by the voter's final
 * choice alone (prediction.py:293-329): no camera that is solved depends on them.  A frame therefore has at most S = 1 + 5 T distinct
 * cameras, T = n_conf_threshs (iterative_voter) or 1 (voter, its threshold is cfg->conf_thresh), and every grid point is a choice among them.
 *   algorithm     0 (iterative_voter) or 2 (voter).  1, 3 and 4 never read the two parameters: SNCAL_ERR_ARG, the message says so.
 *                 cfg->max_rmse and cfg->max_rmse_rel are ignored.
 *   d_grid        (n_grid,2) fp64 rows [max_rmse, max_rmse_rel], 1 <= n_grid <= 4096; NaN and infinities compare as they do in the solve
 *   d_outcomes    (B,S) sncal_camera.  Slot 0: the camera of the first (original_voter) pass -- status 0 when the frame went on to the
 *                 voter, always for algorithm 2.  Slot 1 + 5 t + k: camera k of threshold t in the order rel, acc, all, ground, hom, written
 *                 as sncal_calibrate writes it when the selection takes it (status 3, 4, 5, 6, 7; its own rmse and n_points).  A slot no grid
 *                 point can take is the all-zero record: a solve that failed, a camera good_camera refuses, and every slot of a threshold
 *                 whose voter raises or that lies behind such a threshold.
 *   d_choice      (n_grid,B) int32: the slot grid point g takes for frame b, -1 = no camera (the all-zero record).
 * For every g and b, d_outcomes[b][d_choice[g][b]] equals byte for byte what sncal_calibrate_ws writes for frame b when cfg carries grid
 * point g (tests/test_sweep_gpu.py).  The cameras come from the kernels of sncal_calibrate's default path, unchanged; the remarks there on
 * RANSAC sampling and on parity with OpenCV apply as they stand.
 * Caller-owned workspace of sncal_calibrate_sweep_workspace bytes, 16-byte aligned (SNCAL_ERR_WORKSPACE when short); nothing is launched
 * after an argument error; B == 0 returns SNCAL_OK without touching a pointer.  Asynchronous on `stream`.
 * NOT swept: conf_thresh(s), min_points*, reliable_thresh and min_focal_length decide which points a solve sees -- they change the solves. */
int sncal_calibrate_sweep_workspace(int B, const sncal_voter_cfg* cfg, int n_grid, size_t* bytes);
int sncal_calibrate_sweep(const float* d_kpts, const float* d_line_pts, int B, const sncal_voter_cfg* cfg,
                          const double* d_grid, int n_grid, sncal_camera* d_outcomes, int32_t* d_choice,
                          void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * H2 / N2  batched camera evaluation (accuracy@t of the SoccerNet calibration benchmark)
 * replaces get_polylines / distance_to_polyline / evaluate_camera_prediction and the mirrored-label accuracy choice
 *          baseline/evaluate_camera.py:14-229, 293-320 (the inner loop of src/models/hrnet/metrics.py:97-229)
 *          (sncal_evaluate_outcomes / sncal_sweep_fold below: the same evaluation for the outcome sets of sncal_calibrate_sweep)
 *   d_cams (B) solved cameras (status 0 = missed frame); d_field (n_pts,3) fp64 sampled pitch model in class order,
 *   d_class_start (n_cls+1) int32, d_mirror (n_cls) int32 = index of the left/right-symmetric class
 *   (SoccerPitch.symetric_classes); d_gt (B,n_cls,max_gt,2) fp64 annotated points in pixels with counts
 *   d_gt_cnt (B,n_cls); d_gt_extra (B) = annotated classes outside the pitch model (always false negatives).
 *   d_out (B,12) fp32: confusion [TP,FP,FN,0] with plain labels, the same with mirrored labels, accuracy plain,
 *   accuracy mirrored, chosen pass (1 or 2), evaluated flag (0 for a missed frame).
 * The principal point is (img_w/2, img_h/2) as in Camera.from_json_parameters / project_point.
 * ---------------------------------------------------------------------------------------------- */
int sncal_evaluate_cameras(const sncal_camera* d_cams, int B, const double* d_field, const int* d_class_start,
                           const int* d_mirror, int n_cls, const double* d_gt, const int* d_gt_cnt,
                           const int* d_gt_extra, int max_gt, double threshold, int img_w, int img_h,
                           float* d_out, void* stream);
/* The same evaluation with the per-class outputs of evaluate_camera_prediction (evaluate_camera.py:172-226), both
 * optional:  d_err (B,2,n_cls,max_gt) fp64 = `dict_errors`: distance of annotated point k to the predicted polyline
 * of class c, [b][0] plain labels, [b][1] mirrored labels (the points come from class mirror[c]); NaN = no such
 * point or class not predicted.  d_class_conf (B,2,n_cls,4) int32 = `per_class_confusion` entries
 * {[0,0] points within the threshold, [0,1] points beyond it, [1,0] points of an annotated class that was not
 * predicted, flag: class predicted but not annotated -- the reference books 2 (lines) or 9 (circles) at [0,1]}. */
int sncal_evaluate_cameras_detail(const sncal_camera* d_cams, int B, const double* d_field, const int* d_class_start,
                                  const int* d_mirror, int n_cls, const double* d_gt, const int* d_gt_cnt,
                                  const int* d_gt_extra, int max_gt, double threshold, int img_w, int img_h,
                                  float* d_out, double* d_err, int* d_class_conf, void* stream);
/* The evaluation of sncal_calibrate_sweep's outcome sets: d_outcomes (B,S) candidate cameras, each evaluated against ITS FRAME's
 * annotations (the tables are those of sncal_evaluate_cameras, ONE set per frame, not per slot).  d_contrib (B,S,8) fp64 = what
 * EvalAImetric accumulates for one frame (metrics.py:185-207) should that camera be the frame's: [missed, accuracy of the kept pass,
 * evaluated, tp, tp + fp, tp + fn, sum of the point distances over the classes both predicted and annotated -- class by class, point by
 * point --, number of those points]; a slot with status 0 gives [1,0,0,0,0,0,0,0].  The per-point detail never leaves the workgroup. */
int sncal_evaluate_outcomes(const sncal_camera* d_outcomes, int B, int S, const double* d_field, const int* d_class_start,
                            const int* d_mirror, int n_cls, const double* d_gt, const int* d_gt_cnt,
                            const int* d_gt_extra, int max_gt, double threshold, int img_w, int img_h,
                            double* d_contrib, void* stream);
/* d_acc (n_grid,8) fp64: acc[g] = sum over b of d_contrib[b][d_choice[g][b]] ([1,0,0,0,0,0,0,0] for -1), summed in frame order without
 * atomics: the same bits every run. */
int sncal_sweep_fold(const double* d_contrib, const int32_t* d_choice, int B, int S, int n_grid, double* d_acc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N3  input stage: JPEG bytes -> BGR uint8 frames on the device
 * replaces cv2.imread(path)            src/utils/make_submit.py:62, src/utils/export_line_result.py:176
 *          (opencv-python==4.7.0.72, requirements.txt:5 -> libjpeg-turbo defaults: JDCT_ISLOW, fancy upsampling)
 * The serial part of a JPEG -- marker parsing and Huffman decoding -- runs on host threads into pinned memory;
 * everything with pixel parallelism runs on the device, bit-exactly as libjpeg-turbo computes it: dequantisation +
 * jidctint.c jpeg_idct_islow (samples saturated to 0..255, as its SIMD forms do where jdmaster.c's clamp table would wrap),
 * jdsample.c h2v2/h2v1 fancy upsampling, jdcolor.c YCbCr->RGB.  The output (B,H,W,3) BGR
 * is the input of sncal_hrnet_forward_u8.
 * Supported: 8-bit sequential DCT (SOF0/SOF1), Huffman, one interleaved scan, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
 * restart intervals, 0xFF fill bytes in front of markers.  A scan that ends early (with or without EOI) is decoded as libjpeg
 * does: the MCU in which the data runs out is finished on zero bits, every later MCU keeps zero coefficients (flat grey) -- up to
 * the next restart marker where the one due is in place, else to the end of the frame.
 * Progressive / arithmetic / CMYK / 4:4:0 / multi-scan -> SNCAL_ERR_UNSUPPORTED; streams damaged inside their data (a wrong or
 * missing restart marker, an invalid Huffman code, a coefficient index beyond 63) -> SNCAL_ERR_ARG; the message names the frame.  A file whose EXIF orientation tag asks for a rotation / flip (cv2.imread applies it)
 * -> SNCAL_ERR_UNSUPPORTED as well: the decoder never returns pixels cv2.imread would not.
 * Scaled decode (sncal_jpeg_create_scaled, scale_denom d = 2, 4, 8): libjpeg's own scale_num / scale_denom = 1 / d with every
 * other default kept, i.e. the array cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8) returns, ceil(H / d) x ceil(W / d).
 * The frame is shrunk in the DCT domain (jidctred.c: 4x4, 2x2, 1x1 inverse transforms of the same coefficients; jdmaster.c
 * transforms the chroma of a subsampled frame one size larger instead of upsampling it; jdsample.c upsamples what is left, with
 * the triangle filter at 1/2 and 1/4 and by replication at 1/8) and is bit-exact as well.  It is NOT cv2.resize of the full
 * decode.  The host stage is the same at every scale (libjpeg entropy-decodes everything too); the device stage shrinks.
 * ---------------------------------------------------------------------------------------------- */
typedef struct sncal_jpeg sncal_jpeg;
typedef struct {
    int32_t width, height;
    int32_t components;          /* 1 (grey) or 3 (YCbCr) */
    int32_t h_samp, v_samp;      /* luma sampling factors: 1x1 = 4:4:4, 2x1 = 4:2:2, 2x2 = 4:2:0 */
    int32_t restart_interval;    /* MCUs, 0 = none */
    int32_t blocks[3];           /* 8x8 coefficient blocks per component (MCU padded) */
} sncal_jpeg_info;

/* Host only (no GPU needed): parse the headers of one JPEG. */
int sncal_jpeg_probe(const unsigned char* data, size_t len, sncal_jpeg_info* info);
/* Host only: headers + Huffman decode of one JPEG into quantised coefficient blocks, int16, natural (row-major)
 * order, component after component, each (block_rows, block_cols, 64) -- the layout the device kernels read.
 * `cap` = capacity of `coef` in int16 elements; info->blocks tells how much was written. */
int sncal_jpeg_entropy_decode(const unsigned char* data, size_t len, int16_t* coef, size_t cap,
                              sncal_jpeg_info* info);
/* Decoder for batches of up to max_batch frames of exactly height x width pixels (the reference stacks its frames
 * into one tensor, make_submit.py:63).  n_threads host workers for the entropy decode (0 = hardware concurrency,
 * capped at 32).  Owns pinned staging (double-buffered) and the device coefficient / sample-plane buffers. */
int sncal_jpeg_create(int max_batch, int height, int width, int n_threads, sncal_jpeg** out);
/* The same for frames of height x width SOURCE pixels decoded at 1 / scale_denom (1, 2, 4 or 8; anything else is
 * SNCAL_ERR_ARG).  sncal_jpeg_create is exactly scale_denom = 1. */
int sncal_jpeg_create_scaled(int max_batch, int height, int width, int scale_denom, int n_threads, sncal_jpeg** out);
void sncal_jpeg_destroy(sncal_jpeg* dec);
/* Size of the frames the decoder writes: ceil(height / scale_denom) x ceil(width / scale_denom). */
int sncal_jpeg_output_size(const sncal_jpeg* dec, int* out_h, int* out_w);
/* Host only: the plan of a scaled decode for one header (the one the decoder itself follows).  out_hw = {height, width} of
 * the decoded frame; per component c < info->components: comp_block[c] the side of its inverse transform (8, 4, 2, 1),
 * comp_hw[c] = {height, width} of its sample plane, comp_up[c] = {vertical, horizontal} upsampling left to do (1 or 2).
 * Entries of absent components are 0. */
int sncal_jpeg_scaled_layout(const sncal_jpeg_info* info, int scale_denom, int32_t out_hw[2], int32_t comp_block[3],
                             int32_t comp_hw[3][2], int32_t comp_up[3][2]);
/* data[b], len[b]: host pointers to B encoded frames.  d_bgr: (B,out_h,out_w,3) uint8 on the device (the source size at
 * scale 1).  A frame whose SOURCE size is not the decoder's is refused.  The host part runs inside the call; the copy and
 * the two kernels are enqueued on `stream`. */
int sncal_jpeg_decode(sncal_jpeg* dec, const unsigned char* const* data, const size_t* len, int B,
                      unsigned char* d_bgr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * N4 (heatmap half)  training-target synthesis
 * replaces HRNetLoss.create_target = create_heatmaps + background channel     src/models/hrnet/loss.py:7-52, 81-87
 *   d_kpts (B,N,3) fp32 [x, y, visibility] in heatmap pixels (already divided by the loss stride, loss.py:92)
 *   d_out  (B,N+1,h,w) fp32: N separable amplitude-1 Gaussians (zero where the point is not "visible" by the
 *          reference's own test any(keypoints == 1, dim=-1), loss.py:49) and 1 - max over them as channel N.
 * ---------------------------------------------------------------------------------------------- */
int sncal_create_target(const float* d_kpts, int B, int N, float sigma, int h, int w, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Validation loss, fused: one read of the heatmap, the target rebuilt on the fly (never written)
 * replaces HRNetLoss.forward for num_refinement_stages = 0        src/models/hrnet/loss.py:89-119, 129-144
 *   d_logp (B,N+1,h,w) fp32 log-probabilities (the forward's heat output)
 *   d_kpts (B,N,3) fp32 [x, y, flag] in IMAGE pixels, as the dataset yields them: x and y are divided by `stride` in fp32 here
 *          (loss.py:92) and the visibility test any(keypoints == 1) runs on the divided values
 *   d_mask (B,N+1) fp32 or NULL; multiplied into prediction and target (loss.py:94-103): a channel with mask 0 has exp(0) = 1
 *          against target 0
 *   terms  bit0 MSE sum of (exp(p) - t)^2, bit1 KL sum of xlogy(t, t) - t*p, bit2 adaptive wing (alpha 2.1, omega 14, epsilon 1,
 *          theta 0.5); terms whose bit is clear are not computed and come back 0
 *   d_out  (B,3) fp64: per-frame SUMS over (N+1)*h*w of the three terms.  The caller weighs and divides:
 *          l2_w * S_mse / (B*(N+1)*h*w) + kldiv_w * S_kl / B + awing_w * S_awing / (B*(N+1)*h*w)
 *   d_ws   caller-owned scratch of sncal_heatmap_loss_workspace bytes, 16-byte aligned (SNCAL_ERR_WORKSPACE when short)
 * N <= 64.  Deterministic: no atomics, partial sums are folded in a fixed order, two runs give the same bits.  Asynchronous on
 * `stream`; the library allocates nothing.
 * ---------------------------------------------------------------------------------------------- */
int sncal_heatmap_loss_workspace(int B, int N, int h, int w, size_t* bytes);
int sncal_heatmap_loss(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w, float sigma,
                       float stride, int terms, double* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient of that loss with respect to the log-probabilities: one more read of the heatmap, one write of the gradient
 * replaces torch autograd through HRNetLoss.forward                src/models/hrnet/loss.py:89-144
 *   d_logp, d_kpts, d_mask, sigma, stride, terms   as for sncal_heatmap_loss; the target is rebuilt and not differentiated
 *   coef   HOST array read inside the call: the weight of each term over its divisor,
 *          l2_w / (B*(N+1)*h*w), kldiv_w / B, awing_w / (B*(N+1)*h*w); rounded to fp32 once
 *   d_gout device fp32 scalar, the upstream gradient (a GradScaler's factor needs no host sync), or NULL for 1
 *   d_grad (B,N+1,h,w) fp32 = gout * sum_k coef_k * term_k, per element with m the mask entry, e = exp(x*m), t = target*m:
 *          MSE 2(e - t) e m;  KL -t m;  adaptive wing w'(|t - e|) sign(e - t) e m, where w'(d) = omega a d^(a-1) / (1 + d^a) for
 *          d < theta and A(t) otherwise, a = alpha - t, and sign(0) = 0.  A term whose bit is clear is not evaluated.
 *   d_ws   scratch of sncal_heatmap_loss_workspace bytes (only its tables' share is used), 16-byte aligned
 * Limits and statuses of sncal_heatmap_loss.  No atomics and no reduction: two runs give the same bits.  Asynchronous on `stream`.
 * ---------------------------------------------------------------------------------------------- */
int sncal_heatmap_loss_grad(const float* d_logp, const float* d_kpts, const float* d_mask, int B, int N, int h, int w,
                            float sigma, float stride, int terms, const double coef[3], const float* d_gout,
                            float* d_grad, void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Line model, validation tail: target maps, fused loss, accuracy counts
 *
 * sncal_line_target replaces EHMDataset._generate_keypoint_maps / _add_gaussian      src/models/line/dataset.py:107-178
 *   d_kpts (B,C,2,3) fp32 rows [x, y, flag] in IMAGE pixels, as the dataset yields them; a row with flag == 1 is drawn
 *   d_out  (B,C,h,w) fp32.  Per drawn point mu = (min(w-1, rint(x/stride)), min(h-1, rint(y/stride))): fp32 division, ties to
 *          even, no lower clamp (mu may be negative); exp(-((X-mu_x)^2 + (Y-mu_y)^2) / (2 sigma^2)) divided by its maximum over
 *          the grid (1 unless mu is off the grid); a channel is the sum of its Gaussians, first point first
 *
 * sncal_line_loss replaces EHMLoss.forward for num_refinement_stages = 0              src/models/line/loss.py:34-108
 *   d_pred   (B,C,h,w) fp32, the softmax output of the line head; read once
 *   d_target (B,C,h,w) fp32 maps as a loader delivers them, or NULL
 *   d_kpts   (B,C,2,3) as above, or NULL: the target is rebuilt in registers with target_sigma / stride and never written; the
 *            values and their order are exactly those sncal_line_target writes.  Exactly one of d_target, d_kpts is non-NULL.
 *   terms    bit0 GMSE sum of d^2 * exp(-d^2 / (2 gmse_sigma^2)), d = pred - target; bit1 adaptive wing (alpha 2.1, omega 14,
 *            epsilon 1, theta 0.5); a term whose bit is clear is not computed and comes back 0
 *   d_out    (B,2) fp64: per-frame SUMS over C*h*w.  The caller weighs and divides:
 *            gmse_w * S_gmse / (B*C*h*w) + awing_w * S_awing / (B*C*h*w)
 *   d_ws     caller-owned scratch of sncal_line_loss_workspace bytes, 16-byte aligned (SNCAL_ERR_WORKSPACE when short)
 * C <= 64.  Deterministic: no atomics, partial sums are folded in a fixed order.
 *
 * sncal_line_acc_counts replaces AccMetric.a_t_score's counting                       src/models/line/metrics.py:53-103
 *   d_gt, d_pred (B,C,2,3) fp32; ts: n_t <= 8 distance thresholds, a HOST array read inside the call
 *   d_out (n_t,3) int64 [tp, fp, fn] over the whole batch.  Per (b, c) and slot i: gt_exists = gt[i,2] == 1,
 *   pred_exists = pred[i,2] >= p_threshold, within = min_j |gt[i,:2] - pred[j,:2]| <= t over BOTH predicted points;
 *   tp += gt & pred & within, fn += gt & ~pred, fp += pred & ~gt, fp += gt & pred & ~within (the reference's pairing by slot)
 *
 * sncal_ehm_loss_grad replaces torch autograd through EHMLoss.forward                src/models/line/loss.py:61-108
 *   (named after the class: tests/test_validate_line_host.py pins the set of sncal_line_* names to the validation tail's five)
 *   d_pred, d_target / d_kpts, target_sigma, stride, gmse_sigma, terms   as for sncal_line_loss; the target is not differentiated
 *   coef     HOST array read inside the call: gmse_w / (B*C*h*w), awing_w / (B*C*h*w); rounded to fp32 once
 *   d_gout   device fp32 scalar, the upstream gradient, or NULL for 1
 *   d_grad   (B,C,h,w) fp32 = gout * sum_k coef_k * term_k with d = pred - target, u = d^2 / (2 gmse_sigma^2):
 *            GMSE 2 d exp(-u) (1 - u);  adaptive wing w'(|d|) sign(d), w' as in sncal_heatmap_loss_grad, sign(0) = 0
 *   d_ws     scratch of sncal_line_loss_workspace bytes when d_kpts is given (only its tables' share is used); unused with d_target
 *   Fed sncal_line_target's output as d_target it writes the bits the d_kpts form writes.  No atomics, no reduction.
 *
 * All four are asynchronous on `stream`; the library allocates nothing.
 * ---------------------------------------------------------------------------------------------- */
int sncal_line_target(const float* d_kpts, int B, int C, float sigma, float stride, int h, int w, float* d_out, void* stream);
int sncal_line_loss_workspace(int B, int C, int h, int w, size_t* bytes);
int sncal_line_loss(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w, float target_sigma,
                    float stride, float gmse_sigma, int terms, double* d_out, void* d_ws, size_t ws_bytes, void* stream);
int sncal_ehm_loss_grad(const float* d_pred, const float* d_target, const float* d_kpts, int B, int C, int h, int w,
                         float target_sigma, float stride, float gmse_sigma, int terms, const double coef[2],
                         const float* d_gout, float* d_grad, void* d_ws, size_t ws_bytes, void* stream);
int sncal_line_acc_counts(const float* d_gt, const float* d_pred, int B, int C, float p_threshold, const float* ts, int n_t,
                          long long* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-time augmentation, fused: colour, noise, flip, and the uint8 / fp32 CHW output in one pass
 * replaces ColorAugment, GaussNoise, Flip (image side), ToTensor      src/models/hrnet/transforms.py:16-68, 122-133
 *          (the line model's copies: src/models/line/transforms.py:10-139)
 *   d_src    (B,H,W,3) uint8, the JPEG stage's output
 *   d_params DEVICE array of B entries: one frame's draws, made on the host in the reference's order (augment.py)
 *   d_noise  (B,H,W,3) fp64 normals in SOURCE coordinates (read only for frames with the noise flag), or NULL;
 *            it may not overlap an output (SNCAL_ERR_ARG), and a base off a 16-byte boundary selects the narrow path
 *   d_dst    (B,H,W,3) uint8 or NULL;  d_chw (B,3,H,W) fp32 or NULL = ToTensor: float(v) / 255.0f, the correctly rounded division
 *            that torch.div is on the host, where the reference's ToTensor runs (on the device torch multiplies by
 *            float32(1 / 255) instead, which differs in the last bit for 126 of the 256 byte values).  At least one is non-NULL; requested together they hold the same values.
 * Each frame passes the reference's stages in the reference's order, each gated by its flag, with the reference's uint8
 * truncation between them:
 *   colour   p = double(x) * gain[c];  v = (p - mean[c]) * contrast + mean[c];  clip to [0, 255];  truncate -- fp64 in numpy's
 *            operation order, no contraction.  mean[c] = double(S_c) * gain[c] / double(H*W) with S_c the EXACT integer sum of the
 *            channel (a first kernel, no atomics); numpy sums the rounded products instead, which moves the mean by parts in 1e12
 *            and can change a truncated value only where v lies that close to an integer.
 *   noise    d_noise given: v = double(u8) + d_noise[b,y,x,c], clip, truncate toward zero (fp64): the reference's arithmetic on the
 *            caller's normals.  d_noise NULL: v = float(u8) + float(noise_sigma) * z, clip, truncate (fp32), z from the device
 *            generator below.
 *   flip     out[b, y, W-1-x, :] = v[b, y, x, :]                                                       (cv2.flip(img, 1))
 * Device noise -- a KNOWN DEVIATION from the reference's numbers, like the RANSAC sampling of sncal_calibrate above: GaussNoise draws
 * H*W*3 doubles from numpy's MT19937 stream, which a device cannot replay in parallel.  Here z comes from Philox4x32-10 keyed by
 * the frame's `seed`; the counter is the index of the element quad in the frame's flat SOURCE order (element (y*W + x)*3 + c, four
 * per counter); Box-Muller in fp32 turns the four uniforms into four normals (|z| < 5.8).  A frame's noise depends on its seed and on
 * its pixels' source positions and on nothing else: not on its place in the batch, the tiling, the pointers' alignment or the flip
 * flag.  Same distribution, other numbers.
 * d_src may not overlap an output (SNCAL_ERR_ARG): the flip reads and writes different columns.  B == 0 returns SNCAL_OK without
 * touching a pointer.  d_ws: sncal_augment_workspace bytes, 16-byte aligned (SNCAL_ERR_WORKSPACE when short).  16-byte aligned
 * pointers and W % 16 == 0 take 16-byte accesses; anything else takes a byte path that writes the same bits.  H*W*3 < 2^31,
 * B <= 65535.  Asynchronous on `stream`; the library allocates nothing; no atomics, two runs give the same bits.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {            /* one frame's draws; what the reference takes from random / np.random */
    double gain[3];         /* ColorAugment: brightness * color[c], in the frame's channel order   */
    double contrast;
    double noise_sigma;     /* GaussNoise: the value drawn by np.random.uniform(0, sigma_sq), used as the scale */
    uint64_t seed;          /* device noise stream of this frame */
    uint32_t flags;         /* bit0 colour, bit1 noise, bit2 flip */
    uint32_t reserved;
} sncal_augment_params;

int sncal_augment_workspace(int B, int H, int W, size_t* bytes);
int sncal_augment_u8(const unsigned char* d_src, int B, int H, int W, const sncal_augment_params* d_params,
                     const double* d_noise, unsigned char* d_dst, float* d_chw,
                     void* d_ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pipeline plumbing: a stream confined to `cus_per_xcd` compute units of each XCD (for the camera solves)
 * replaces the 16-process CPU pool of make_submit.py:25,53-54,69 (ProcessPoolExecutor workers beside the GPU loop): the solves of
 * up to four batches run beside the network on these streams; what they may occupy is bounded by the mask instead of by a process
 * count.  BLOCKING stream (synchronises with the legacy null stream): see csrc/api.cpp.  Destroy with sncal_stream_destroy.
 * ---------------------------------------------------------------------------------------------- */
int sncal_stream_create_cu_mask(int cus_per_xcd, void** stream);
int sncal_stream_destroy(void* stream);

/* ------------------------------------------------------------------------------------------------
 * Keypoint labels: SoccerNet line / circle annotations -> the 57 keypoint labels of a batch, one launch
 * replaces get_intersections                       src/datatools/intersections.py:104 (with ellipse.py:275-516 behind it)
 *          HRNetDataset._annot2keypoints           src/models/hrnet/dataset.py:73-87  (the [x, y, 1] / [-1, -1, 0] rows and the mask)
 *          FixLRAmbiguous (with SNCAL_LABELS_FIX_LR) src/models/hrnet/transforms.py:136-186
 * The specification is this build's host restatement, annotations.get_intersections: same stages, same decisions; fp64.
 *   d_points   (total_points, 2) fp64, NORMALISED image coordinates as annotated, the frames' classes one after the other
 *   d_offsets  (B, n_classes + 1) int32: frame b's class c owns points [d_offsets[b][c], d_offsets[b][c + 1]); a range that leaves
 *              [0, total_points] reads as an empty class.  n_classes = 28, the class order is fixed:
 *                0 Circle central, 1 Circle left, 2 Circle right,
 *                3..25 the 23 line classes in LINE_CLS order (src/datatools/line.py:35-57): Goal left post left , Goal right post
 *                right, Middle line, Small rect. right top, Side line bottom, Goal right post left, Big rect. right main, Goal left
 *                crossbar, Small rect. left bottom, Side line left, Big rect. right top, Small rect. left top, Side line right, Big
 *                rect. left top, Goal left post right, Small rect. right bottom, Side line top, Goal right crossbar, Small rect. left
 *                main, Big rect. left main, Big rect. right bottom, Small rect. right main, Big rect. left bottom,
 *                26 Goal unknown, 27 Line unknown (carried, read by no label)
 *   d_present  (B) uint32: bit c set = class c is a KEY of the frame's annotation (an empty polyline still counts: FixLRAmbiguous
 *              counts names, pick_side walks them)
 *   img_w, img_h, within_image, margin   get_intersections' img_size, within_image, margin
 *   num_keypoints  N <= 57: rows and mask entries written per frame
 *   flags      SNCAL_LABELS_FIX_LR: labels at margin 0 first, FixLRAmbiguous.decide on them (threshold 10), d_swapped[b] = its verdict;
 *              a swapped frame's outputs are those of the annotation renamed by flip_annot_names(swap_top_bottom=False,
 *              swap_posts=False) -- a fixed permutation of the class ids -- at the caller's margin
 *   d_samples  (54, 200, 4) uint8: at index n (5 <= n <= 53) the 200 index quadruples numpy draws for n correspondences with
 *              Generator(PCG64(12345)).choice(n, 4, replace=False), the host RANSAC's sequence (annotations.ransac_samples); entries
 *              below 5 are not read (4 correspondences are one hypothesis on 0..3).  An index >= n is clamped to n - 1.
 *   d_keypoints (B, 3N) fp32 rows [x, y, 1], or [-1, -1, 0] for an absent label;  d_mask (B, N + 1) int64 ones, zero at the ids
 *              30..56 that neither the circles nor the homography produced
 *   d_labels   (B, 57, 2) fp64 labels before the fp32 rounding (NaN where absent) with d_label_present (B, 57) bytes, or both NULL
 *   d_swapped  (B) bytes; may be NULL without the flag
 *   d_ws       sncal_keypoint_labels_workspace bytes (0 in this version: a frame's state lives in its workgroup's LDS and polylines
 *              of any length are read where they lie); may be NULL when that is 0
 * Degenerate 4-point samples: exactly three collinear PITCH points give the host's DLT one exact solution, the rank-one d4 l^T
 * (every point off the line l lands on the fourth point's image, a point on it is 0 / 0 = NaN), which is restated; it decides a
 * frame only when it is the one hypothesis of n == 4.  Declared deviations from the host path, rounding apart: any other degenerate
 * sample (four collinear pitch points, collinear image points) is skipped, where the host's SVD returns a vector of a null space of
 * more than one dimension; the ellipse's eigenvector comes from the characteristic cubic, so a fit whose 3x3 has a complex pair is
 * judged on its real eigenvector alone.
 * One wavefront per frame, plain stores, no atomics: two runs write the same bits.  B == 0 returns SNCAL_OK without touching a
 * pointer.  Asynchronous on `stream`; the library allocates nothing.
 * ---------------------------------------------------------------------------------------------- */
#define SNCAL_LABELS_FIX_LR 1u
int sncal_keypoint_labels_workspace(int B, int total_points, size_t* bytes);
int sncal_keypoint_labels(const double* d_points, int total_points, const int* d_offsets, const unsigned* d_present, int B,
                          int n_classes, int img_w, int img_h, int within_image, double margin, int num_keypoints,
                          unsigned flags, const unsigned char* d_samples, float* d_keypoints, long long* d_mask,
                          double* d_labels, unsigned char* d_label_present, unsigned char* d_swapped, void* d_ws,
                          size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Extremity metric: detected line ends against the annotation, per frame, a batch and n_t thresholds in one launch
 * replaces evaluate_detection_prediction and the two-labelling choice    baseline/evaluate_extremities.py:37-116, 192-216
 *          scale_points                                                  baseline/evaluate_extremities.py:119-134
 *          get_line_data's `points` (peaks form)                         src/utils/export_line_result.py:115-124
 * (named after the metric, not the line model: tests/test_validate_line_host.py pins the set of line-model entry points)
 *   d_gt_points, total_points, d_gt_offsets   the annotations, packed as sncal_keypoint_labels takes them: (total_points, 2) fp64
 *              normalised, (B, n_classes + 1) int32 offsets, n_classes = 28 in that entry point's class order.  A class with at least
 *              one point counts n = its point count; its first and last point are multiplied by (img_w - 1, img_h - 1).  A class
 *              without points, or whose range leaves [0, total_points], is absent.
 *   the prediction, exactly one of two forms:
 *     d_peaks  (B, C, 2, 3) fp32 rows [x, y, p] in map cells, channel k = class 3 + k (LINE_CLS order), C <= 23.  Slot i is kept when
 *              p >= p_threshold; its pixel is (x * scale, y * scale) in fp32, widened; n = kept slots (0 = absent), slot order kept,
 *              one kept slot is both first and last.  (Rows that are pixels already -- sncal_line_decode with its scale -- take scale 1.)
 *     d_pred_points, pred_total, d_pred_offsets   packed and scaled like the annotations (the extremities_<id>.json files)
 *   ts         HOST array of n_t <= 8 pixel thresholds, read inside the call
 * 'Circle central' (class 0) is removed from both sides.  'Goal unknown' and 'Line unknown' are not: annotated, they are false
 * negatives, as in the reference.  Per frame two labellings: prediction class c against annotation class c (0), or against the
 * point-symmetric class (1: mirror_labels on the annotation).  Under each: a class only detected adds fp += n_pred, a class only
 * annotated adds fn += n_gt (under the prediction-side name), a class on both sides takes d1 = |gt first - pred first|,
 * d2 = |gt last - pred last| -- or the crossed pair when both crossed distances are <= -- and each adds tp when < t, else fp.
 * acc = float32(tp) / float32(tp + fp + fn), 0 for an empty frame; labelling 0 is kept only when acc0 > acc1 (a tie is mirrored),
 * per threshold.  Of the kept labelling:
 *   d_frame (n_t, B, 4) int32 [tp, fp, fn, labelling];  d_class (n_t, B, 28, 3) int32 [tp, fp, fn] per prediction-side class;
 *   d_err (n_t, B, 28, 2) fp64 [d1, d2], NaN where the class is not on both sides.
 * Counts are exact below 2^24 per frame (the reference's confusion matrix is float32).  One wavefront per frame, plain stores, no
 * atomics: two runs write the same bits.  B == 0 returns SNCAL_OK without touching a pointer.  Asynchronous on `stream`; the
 * library allocates nothing.
 * ---------------------------------------------------------------------------------------------- */
int sncal_extremity_counts(const double* d_gt_points, int total_points, const int* d_gt_offsets, const float* d_peaks, int C,
                           float scale, float p_threshold, const double* d_pred_points, int pred_total, const int* d_pred_offsets,
                           int B, int n_classes, int img_w, int img_h, const double* ts, int n_t, int* d_frame, int* d_class,
                           double* d_err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cameras from line extremities: the dev-kit's baseline of the calibration task, per frame, a batch in one launch
 * replaces the per-frame body of __main__                                baseline/baseline_cameras.py:174-246
 *          normalization_transform                                       baseline/baseline_cameras.py:13-41
 *          estimate_homography_from_line_correspondences                 baseline/baseline_cameras.py:44-106
 *          Camera.from_homography, project_point, refine_camera          baseline/camera.py:121-154, 249-268, 105-119
 * (named after the reference's file: tests/test_validate_line_host.py and tests/test_extremities_host.py pin the sets of line-model and
 *  extremity-metric entry points)
 *   the prediction, exactly one of two forms (those of sncal_extremity_counts):
 *     d_peaks  (B, C, 2, 3) fp32 rows [x, y, p], channel k = class 3 + k (LINE_CLS order), C <= 23.  A class is kept when BOTH slots
 *              have p >= p_threshold.  A pixel is float32(x * scale), widened, divided by (img_w - 1, img_h - 1) -- the value an
 *              extremities_<id>.json of this package holds -- and multiplied by (img_w, img_h) as the baseline reads such a file: the
 *              same bits as the route through the files.
 *     d_pred_points, pred_total, d_pred_offsets   (pred_total, 2) fp64 normalised points and (B, n_classes + 1) int32 offsets,
 *              n_classes = 28 in sncal_keypoint_labels' class order.  A class contributes its first two points, times (img_w, img_h)
 *              (:188-189: the size, not the size - 1); with fewer than two points, or a range that leaves [0, pred_total], it is
 *              skipped (the reference raises IndexError there).
 *   Classes are walked in class order; 'Circle central' and the two 'unknown' classes are skipped.  A kept class appends its two image
 *   points to the candidates of its two 3-D end points (end points shared between lines merge) and to the image cloud; its line
 *   p1 x p2 joins the line matches when its coefficients sum to a finite number and the class lies on the lawn (no post, no crossbar,
 *   no circle).  Fewer than 4 line matches: no camera.  Else: both clouds normalised (the running mean of :22-29), the 2L x 9 system
 *   of :53-84, its SVD (one-sided Jacobi on the wave; A^T A is never formed) and the right singular vector at index min(2L, 9) - 1
 *   of the singular values sorted descending, walking up past exact zeros (:87-97) -- with exactly four lines that is the vector of
 *   the smallest of EIGHT values, not the null vector: the reference's behaviour, kept.  H = inv(T2) V T1 / H[2][2]; focal length
 *   from the image of the absolute conic, the nearest rotation of [r0 r1 r0 x r1], the position; every 3-D end point that projects
 *   strictly inside the image takes its nearest candidate (the first of equal ones) when closer than 100 px; with more than 3 such
 *   matches and refine = 1 the pose is refined by the LM of sncal_pnp_refine_lm (same schedule, cap and stop; SNCAL_SOLVE_SCHEDULE
 *   applies as there).  refine = 0 stops after from_homography.
 *   d_cameras (B) the camera, n_points = matches, rmse = mean L2 over the matches (0 without any), status as d_status;
 *   d_status (B) int32 SNCAL_LINECAM_*;  d_H (B, 9) fp64 the homography, zeros when none was estimated or it is not finite;
 *   d_n_lines (B) int32 line matches;  d_slots (B, n_slots = 34) int32: per 3-D end point (the distinct end points of the lines,
 *   sorted by keypoint id) the chosen candidate as class * 2 + end, or -1.
 * A frame without a camera has a zeroed record: no output holds a NaN.  One wavefront per frame, plain stores, no atomics: a frame's
 * record depends on neither the batch size nor its position.  B == 0 returns SNCAL_OK without touching a pointer.  Asynchronous on
 * `stream`; the library allocates nothing and needs no workspace.
 * ---------------------------------------------------------------------------------------------- */
enum {
    SNCAL_LINECAM_NONE = 0,        /* fewer than 4 line matches, no singular vector, or from_homography failed          */
    SNCAL_LINECAM_HOMOGRAPHY = 1,  /* Camera.from_homography's camera, not refined (refine = 0, or at most 3 matches)    */
    SNCAL_LINECAM_REFINED = 2      /* refined on its matches                                                             */
};
int sncal_baseline_cameras(const float* d_peaks, int C, float scale, float p_threshold, const double* d_pred_points, int pred_total,
                       const int* d_pred_offsets, int B, int n_classes, int img_w, int img_h, int refine, sncal_camera* d_cameras,
                       int32_t* d_status, double* d_H, int32_t* d_n_lines, int32_t* d_slots, int n_slots, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frames of any size: cv2.resize's bilinear (INTER_LINEAR) on uint8 BGR frames, a batch in one launch
 * replaces cv2.resize(img, (W, H))    src/models/line/dataset.py:73
 *          the dev-kit's copies       baseline/dataloader.py:62, baseline/detect_extremities.py:237
 * The arithmetic is OpenCV 4.7's 8-bit path (modules/imgproc/src/resize.cpp, the C / SIMD code), restated:
 *   taps of one axis, destination index d:  scale = 1.0 / ((double)n_dst / n_src);  f = (float)((d + 0.5) * scale - 0.5) in double
 *     without contraction;  s = floor(f);  f -= s in float;  c0 = rint((1.f - f) * 2048.f), c1 = rint(f * 2048.f) in float, half to
 *     even, int16 (they need not sum to 2048).
 *     x axis (zero_edges = 1): s < 0 -> s = 0, f = 0;  s >= n_src - 1 -> s = n_src - 1, f = 0;  the second column is min(s + 1, w - 1).
 *     y axis (zero_edges = 0): f is kept and the rows s, s + 1 are clipped to [0, n_src - 1] each, so a first row with s = -1 reads
 *     row 0 twice with both weights.
 *   pixel, int32:  h0 = S[y0][x0] * a0 + S[y0][x1] * a1, h1 the same on row y1;
 *                  out = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2              (0..255 without a clamp)
 *   w == 2 W and h == 2 H exactly: cv::resize takes its fast area path instead, (a + b + c + d + 2) >> 2 over the 2x2 block; a ratio
 *   of 2 along one axis only takes the general path.  h == H and w == W is a copy.
 * sncal_resize_tables is HOST ONLY (no GPU): ofs[n_dst] = s (after the x rule; unclipped under the y rule) and coef[n_dst][2] =
 * (c0, c1) of one axis, from the same function the kernel forms its taps with on the device.
 * sncal_resize_u8: d_src (B,h,w,3) uint8 -> d_dst (B,H,W,3) uint8, one pass, no intermediate tensor, no workspace.  B == 0 returns
 * SNCAL_OK without touching a pointer.  SNCAL_ERR_ARG: a dimension < 1, h*w*3 or H*W*3 >= 2^31, B > 65535, overlapping ranges.
 * A 16-byte aligned d_dst with H * W % 16 == 0 takes 16-byte stores; anything else takes a byte path that writes the same bits.
 * Asynchronous on `stream`; the library allocates nothing; vector stores, no atomics: two runs give the same bits.
 * Pinned to a numpy restatement of the formulas above and to float64 bilinear within < 1 level; OpenCV's own bytes are pinned only
 * once tests/test_resize_cv2_optional.py has run with a cv2.
 * ---------------------------------------------------------------------------------------------- */
int sncal_resize_tables(int n_src, int n_dst, int zero_edges, int32_t* ofs, int16_t* coef);
int sncal_resize_u8(const unsigned char* d_src, int B, int h, int w, unsigned char* d_dst, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SNCAL_H */
