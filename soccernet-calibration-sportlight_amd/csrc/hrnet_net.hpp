// Internal header of the HRNet host side: the plan's data (layers, ops, tensors, launch schedule, struct sncal_hrnet) and the functions
// with which its stages call each other (below; hrnet.cpp, the executor and C ABI, calls them).  Included by the hrnet*.cpp units only.
#pragma once
#include "common.hpp"
#include "conv.hpp"
#include "ops.hpp"
#include "head.hpp"
#include "bblock.hpp"
#include "bblockx3.hpp"
#include "bneckx3.hpp"
#include "x3.hpp"
#include "conv_tt.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace sncal {

// A packed-weight buffer on the device and its size: the size the packer's ..._packed_bytes() gave (pack.hpp), the range of the
// buffer descriptor through which the kernel reads it, and what tt_eligible bounds by 2^31
struct DevBuf { void* p = nullptr; size_t bytes = 0; };

enum LayerPacking {      // one per kernel that may read a layer; each format is owned by that kernel's header
    PK_GENERIC,          // conv.hpp: every layer, fragment order of the layer's (MI, G)
    PK_TT,               // conv_tt.hpp, bf16: wide 3x3 stride-1 layers
    PK_TT_FP8,           // conv_tt.hpp, C5 path: e4m3 weights of the same layers, one scale per output channel (wscale); the launch scales by
                         // d_oscale = (calibrated scale of the layer's input tensor) x wscale
    PK_TT_X3,            // conv_tt.hpp, split engine: hi / lo weights in 16-channel stages, output-channel blocks of x3_blk
    PK_BBX3,             // bblockx3.hpp, split engine: pair-step packing of the 48 -> 48 3x3 layers of the fused BasicBlock
    PK_BNP,              // bneckx3.hpp, split engines: layer1's 1x1 layers (64 -> 256, 256 -> 64) for the fused Bottleneck seam
    PK_COUNT
};
enum HeadPacking {       // head.hpp; layout() picks the head variant from which of these exist and from head_ks16
    HPK_W0, HPK_W1,              // head.hip, bf16: 16x16x32 fragments
    HPK_W0_32, HPK_W1_32,        // head32.hip / headx3.hip: 32x32x16 fragments (K1 a multiple of 16); split engines: the hi parts
    HPK_W0_32_LO, HPK_W1_32_LO,  // headx3.hip: the lo parts of the split weights
    HPK_COUNT
};

struct ConvLayer {
    std::string name, bn;
    int cin, cout, k, stride;
    bool bias;
    // host weights (BN folded on set)
    std::vector<float> w, scale, shift;
    bool is_set = false;
    // packing / dispatch
    int cin_phys = 0, mi = 0, g = 0, chunks = 0, nblk = 0, cout_frags = 0;
    DevBuf packed[PK_COUNT];    // null = the layer's shape (or the engine) has no use for that kernel
    float* d_bias = nullptr;
    std::vector<float> wscale;
    float* d_oscale = nullptr;  // allocated with PK_TT_FP8, filled by sncal_hrnet_calibrate_fp8
    int stage = 0;              // 2..4 for model.stageN.* layers, 0 otherwise
    bool fp8_on = false;
    int x3_blk = TT_COUT;       // PK_TT_X3: blocks of 96 (TT_TILE_96x8, TT_TILE_96x4) or, for widths that are no multiple of 96, 64 (TT_TILE_64x12): ttx3_block
    bool x3_on = false;
    // internal layers of the fused head: t_i = W0[:, col_off : col_off + cin] . branch_i  (derived at finalize)
    bool derived = false;
    int col_off = 0;
    bool derived_shift = false;     // the slice that also carries last_layer.0's folded-BN shift (split head: the direct tensor's)
    Folded folded() const { return Folded{w.data(), scale.data(), cout, cin, k}; }
};

enum OpType { OP_INPUT, OP_CONV, OP_UPADD, OP_SOFTMAX, OP_DECODE, OP_HEAD };
enum OpGroup { GRP_ALL = 0, GRP_UNFUSED = 1, GRP_FUSED = 2, GRP_SPLIT = 3 };   // head variants living side by side in the plan

struct Op {
    OpType type;
    int conv = -1;
    int in = -1, out = -1, res = -1;
    bool relu = false;
    int out_coff = 0;
    bool out_f32 = false;
    bool res_twin = false;       // bf16x3: the residual is read from res's split twin (set by layout())
    int base = -1, srcs[4] = {-1, -1, -1, -1}, nsrc = 0;
    int dims_from = -1, dims_mul = 1;     // UPADD without base: out dims = dims(dims_from) * dims_mul
    int group = GRP_ALL;
    int launch_group = -1;                // >= 0: independent convs that may share one grouped launch (consecutive ops)
    bool shared_in = false;               // ... and all members read the SAME input tensor with stride 2 (conv_shared_s2_kernel)
    int head_direct = -1, head_src[HEAD_MAX_SRC] = {-1, -1, -1, -1, -1}, head_nsrc = 0;   // OP_HEAD
    int head_fold[HEADX4_FOLD] = {-1, -1, -1}, head_nfold = 0;                            // OP_HEAD: sources folded into stage-1 K
                                                                                          // (head_direct < 0, upscale 4: the stem leads them)
};

struct Tensor {
    int C = 0;
    bool f32 = false;         // fp32 storage regardless of the net dtype (logits / heat)
    bool external_heat = false;
    bool fp8 = false;            // e4m3 twin (1 byte per element) of a bf16 tensor, input of an fp8 convolution
    bool split = false;          // bf16x3 engine: split twin ([16 hi | 16 lo] bf16 per 16-channel group = 4 bytes per element) of an fp32 tensor
    int twin = -1;               // index of this tensor's fp8 twin, if any
    float scale = 0.f;           // calibrated per-tensor scale of the twin: amax / 448
    int first = -1, last = -1;   // producing / last consuming op, as the allocator sees them (extended over launch groups and fusable pairs)
    int last_read = -1;          // the op that really reads the tensor last (what a fusion's "nobody else reads it" test asks)
    // per-run
    int H = 0, W = 0;
    size_t offset = 0, bytes = 0;
};

// ---- launch schedule: which kernel runs which ops, decided once per (layout, sub-batch size) -------------------------
enum LaunchKind {
    LK_INPUT,        // NCHW fp32 / HWC u8 frames -> NHWC
    LK_CONV,         // one convolution on the generic kernel (conv.hpp)
    LK_TT,           // one to three independent convolutions on the two-team kernel (conv_tt.hip)
    LK_GROUP,        // two or three independent convolutions as one grouped launch of the generic kernel
    LK_SHARED_S2,    // the chain-starting stride-2 convolutions of one input tensor as one launch (conv_shared_s2_kernel)
    LK_BNECK_TAIL,   // layer1 block 0: downsample branch + conv3 (bneckx3.hip)
    LK_BNECK_SEAM,   // layer1: conv3 of a Bottleneck + conv1 of the next (bneckx3.hip)
    LK_BBLOCKX3,     // 48-channel BasicBlock in split arithmetic (bblockx3.hip)
    LK_BBLOCK48,     // 48-channel BasicBlock, bf16 (bblock.hip)
    LK_UPADD,        // upsample + add (ops.hip)
    LK_HEAD,         // fused head (head.hip / head32.hip / headx3.hip / headx4.hip)
    LK_TAIL,         // softmax, or the part of the keypoint decode fused with it
    LK_DECODE,       // keypoint decode (decode.hip)
};
enum DecodeAt { DEC_NONE, DEC_HEAD, DEC_TAIL };    // where the keypoint decode runs when a call wants keypoints only
enum TwinBy : char { TW_NONE, TW_PRODUCER, TW_FRONT };     // who makes a tensor's twin: nobody (not alive), its producer's epilogue, a helper in front of each reader
enum Prep : char { PREP_NONE, PREP_QUANT_FP8, PREP_SPLIT_F32 };     // the helper (quant.hip) that makes a member's input twin in front of the launch
struct Forms { bool dense = true, twin = false; };         // what a launch writes of an op's output: the tensor itself, its twin

struct Member {                     // what the schedule resolved for one op a launch covers
    const ConvVariant* v = nullptr; // generic kernel: variant, tile width factor, tiles, dynamic LDS bytes, LDS-transposed epilogue
    int twf = 1, tiles_x = 0, tiles_y = 0;
    size_t lds = 0;
    bool epi_lds = false;
    Forms out;                      // the forms of the op's output that the launch writes (neither: it stays in LDS)
    Prep prep = PREP_NONE;          // LK_TT, LK_BBLOCKX3: the helper in front of the launch for this op's input
};
struct TTPlanDev { TTItem* items = nullptr; uint32_t* first = nullptr; int n_wgs = 0; int lazy = 0; TTTile cfg = TT_TILE_96x8; };
struct Prof { std::string kernel; double flops = 0, bytes = 0; };
struct Launch {
    LaunchKind kind = LK_CONV;
    int op = 0, n = 1;              // covers the ops [op, op + n), all active
    Member m[3];
    TTPlanDev plan;                 // LK_TT: work lists (cfg, the tile, set by the schedule; uploaded by the first launch)
    Prof prof, prof_kp;             // profile row; LK_TAIL: prof_kp when the call wants keypoints only
};
struct Schedule {
    int sb = 0;
    DecodeAt dec = DEC_NONE;
    std::vector<TwinBy> twin_by;    // per tensor: who makes its twin at this layout; every fusion predicate and member reads this
    std::vector<Launch> launches;
};

}  // namespace sncal

struct sncal_hrnet {
    sncal_hrnet_desc desc;
    int dtype;
    int ge;          // elements per 16-byte k-group
    int esize;
    std::vector<sncal::ConvLayer> layers;
    std::map<std::string, int> layer_by_name;
    std::vector<sncal::Op> ops;
    std::vector<sncal::Tensor> tensors;
    int t_heat = -1, t_kpts_src = -1;
    int n_public = 0;                 // layers [0, n_public) are the reference's convs; the rest are internal
    int t_stem = -1, t_branch0 = -1;  // tensors whose dims decide whether the fused head applies
    int l_head0 = -1, l_head1 = -1;   // last_layer.0 / last_layer.3
    int head_direct_coff = 0, head_direct_c = 0, head_hp = 0, head_m2 = 0;
    int head_k = 0, head_ks1 = 2;     // stage-1 K of the fused head (direct + folded branch channels), its k-steps
    bool fused_enabled = true, use_fused = false;
    // exact-fp32 engine: the head in its restructured form (per-source 1x1 products at native resolution, one bilinear sum) on the
    // generic fp32 kernels -- the 784 -> 784 product at 270x480 (31 % of the reference's MACs) shrinks ninefold
    bool has_split = false, use_split = false;
    // wide 3x3 stride-1 convolutions (96 / 192 / 384 channels) on the two-team persistent kernel (conv_tt.hip), bf16 path
    bool use_conv_tt = sncal::env_flag(sncal::ENV_CONV_TT);
    std::vector<sncal::Schedule> schedules;      // per sub-batch size at the current layout (SB and the last sub-batch's), dropped with the layout
    int n_cus = 0;                        // compute units of the device (queried at finalize)
    // C5: fp8 (OCP e4m3) arithmetic for the wide 3x3 stride-1 convolutions, everything else as the bf16 engine
    bool fp8 = false, fp8_calibrated = false, calibrating = false;
    // SNCAL_BF16X3: the fp32 engine with split-bf16 arithmetic in the 3x3 stride-1 convolutions of stages 2-4 and in the generic
    // convolutions (x3_t variants: packed weights [4 hi | 4 lo] per k-group); residuals of the two-team convolutions come from split twins
    bool x3 = false;
    unsigned fp8_stages = 0;                  // bit s: stage s selected (0 = all stages)
    std::vector<int> fp8_widths;              // selected channel widths (empty = all)
    unsigned* d_amax = nullptr;               // calibration: per-tensor max |x| (float bit patterns)
    std::vector<char> need_bf16;              // per tensor: some active consumer reads the bf16 tensor
    std::vector<int> producer;                // per tensor: active op that writes it
    bool fuse_bblock = sncal::env_flag(sncal::ENV_FUSE_BBLOCK);   // 48-channel BasicBlocks as one kernel (bblock.hip), bf16 path
    // split engines, layer1 (bneckx3.hip): bit 0 = conv3 of a Bottleneck + conv1 of the next as one pass, bit 1 = block 0's downsample branch inside its conv3
    int fuse_bneck = sncal::env_int(sncal::ENV_FUSE_BNECK);
    sncal::DevBuf head_packed[sncal::HPK_COUNT];
    int head_ks16 = 0;
    float *d_hb0 = nullptr, *d_hb1 = nullptr;
    int cur_group = sncal::GRP_ALL;
    bool finalized = false;
    bool equalize = true;        // fp16x3: rebalance block-internal channels by powers of two at finalize (equalize_blocks)
    bool equalize_done = false;  // ... already applied to the weights held now (re-armed by sncal_hrnet_set_conv)
    int equalized = 0;           // channels moved by the last equalize_blocks
    int subbatch = 64;
    const sncal::ConvVariant* variants = nullptr;
    int nvariants = 0;
    // cached per-(sb,H,W) layout
    int lay_sb = -1, lay_h = -1, lay_w = -1;
    size_t lay_bytes = 0;
    // profiling (sncal_hrnet_set_profiling): events recorded between launches + what each interval ran
    int profiling = 0;                    // 0 off, 1 every launch, 2 only the launches of `focus` (labels cached per op by a mode-1 run)
    std::string focus;
    int n_launch_groups = 0;
    std::vector<std::string> op_label;
    struct Interval { hipEvent_t e0, e1; std::string kernel; double flops, bytes; };
    std::vector<Interval> intervals;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    // work tickets of the persistent kernels that deal their work dynamically (TICKET_*): zeroed words, re-armed by the kernels
    // themselves; launches of one network are ordered on its stream, so they share the words
    unsigned* d_tickets = nullptr;
    // range flag of the split-fp16 engine (x3.hpp x3_report): [0] wavefronts that split a value beyond +-65504, [1] workgroups of the
    // layout kernel that met a NaN / infinite input value.  Sticky until sncal_hrnet_range_status(clear = 1); allocated at finalize
    unsigned* d_range = nullptr;
    // test instrumentation (sncal_hrnet_plan_tap): copies of plan tensors taken while the executor passes an op
    struct Tap { int op, tensor; void* dst; };
    std::vector<Tap> taps;
};

namespace sncal {

inline std::string fmt(const char* f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof(buf), f, ap);
    va_end(ap);
    return buf;
}

// ticket words of a network: the first word of each kernel's own range
constexpr int TICKET_SEAM = 0;       // layer1's seams and block 0's tail (bneckx3.hip)
constexpr int TICKET_BBX3 = 16;      // fused BasicBlock, split arithmetic (bblockx3.hip)
constexpr int TICKET_TT = 32;        // two-team kernel (conv_tt.hip)
constexpr int TICKET_BB48 = 48;      // fused BasicBlock, bf16 (bblock.hip)
constexpr int TICKET_WORDS = 96;

// the head variants live side by side in the plan: is this op part of the variant the current layout chose?
inline bool op_active(const sncal_hrnet& net, const Op& op) {
    const int head = net.use_fused ? GRP_FUSED : net.use_split ? GRP_SPLIT : GRP_UNFUSED;
    return op.group == GRP_ALL || op.group == head;
}

// bytes of sb frames of tensor t in its storage type
inline size_t tensor_bytes(const sncal_hrnet& net, const Tensor& t, int sb) {
    return (size_t)sb * t.H * t.W * t.C * (t.f32 ? 4 : t.fp8 ? 1 : net.esize);
}

// source step per destination pixel of an align_corners = True resize
inline float align_corners_ratio(int src, int dst) { return dst > 1 ? (float)(src - 1) / (float)(dst - 1) : 0.f; }

// ---- the stages: one unit each, what the others call of it, when it runs --------------------------------------------
// hrnet_graph.cpp: the op graph of a network (sncal_hrnet_create)
bool build_graph(sncal_hrnet& net);
// hrnet_weights.cpp: balance, packing and upload of the weights (sncal_hrnet_finalize), release of the packed buffers
int equalize_blocks(sncal_hrnet& net);
int pack_weights(sncal_hrnet& net);
void release_weights(sncal_hrnet& net);
// hrnet_layout.cpp: head variant, shapes, lifetimes, workspace offsets (per sub-batch, H, W)
int layout(sncal_hrnet& net, int sb, int H, int W);
int sub_batch(sncal_hrnet& net, int B, int H, int W);      // frames per sub-batch of a call of B frames
void drop_layout(sncal_hrnet& net);
// hrnet_schedule.cpp: which kernel runs which ops (per layout and sub-batch size), and the predicates layout and launches share
bool tt_eligible(const sncal_hrnet& net, const Op& op, int sb);
void head_params(const sncal_hrnet& net, const Op& op, int sb, HeadParams& hp);
void headx4_params(const sncal_hrnet& net, const Op& op, int sb, HeadX4Params& hp);      // ... of a head without a direct tensor (upscale 4)
int schedule_for(sncal_hrnet& net, int sb, Schedule** out);

}  // namespace sncal
