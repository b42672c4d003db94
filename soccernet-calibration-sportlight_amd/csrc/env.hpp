// Every environment switch libsncal.so reads: one row each, and the three accessors through which the sites read them (api.cpp holds
// the table's expansion and the accessors).  No other unit of csrc/ calls getenv.  README.md ("Environment switches") repeats the
// table for users; tests/test_env_switches_host.py keeps the two, and the sites, in step.
//
// kind      FLAG: unset = the default, "0" = off, anything else = on (env_flag).  INT: atoll of the value (env_int).
//           STR: the value itself, null when unset (env_str).
// lifetime  PROCESS: the accessor reads the variable on its own first call for that row and keeps the value (thread-safe); a change
//           of the variable afterwards is not seen, so a test toggles such a switch in a subprocess.  NET / PLAN / LAUNCH rows are
//           read on every call of the accessor; the word says where the caller calls it -- when a network is created, when a
//           launch schedule is planned for a layout, at every launch -- and with that what an in-process toggle has to rebuild.
#pragma once

namespace sncal {

//        identifier      name                      kind  default      lifetime  what it selects; who sets it
#define SNCAL_ENV_TABLE(X)                                                                                                                   \
    X(CONV_TT,        "SNCAL_CONV_TT",        FLAG, 1,           NET,     "wide 3x3 stride-1 convolutions on the two-team kernel (conv_tt.hip); 0 = the generic kernel; tests (A/B reference)") \
    X(FUSE_BBLOCK,    "SNCAL_FUSE_BBLOCK",    FLAG, 1,           NET,     "bf16 engines: 48-channel BasicBlocks as one kernel (bblock.hip); 0 = two convolutions; tests (A/B reference)") \
    X(FUSE_BNECK,     "SNCAL_FUSE_BNECK",     INT,  3,           NET,     "layer1 fusions of the split engines (bneckx3.hip): bit 0 = the seams, bit 1 = block 0's downsample tail; tests (A/B reference)") \
    X(FUSED_HEAD,     "SNCAL_FUSED_HEAD",     FLAG, 1,           NET,     "the fused head kernels; 0 = the reference's upsample + concat + two 1x1 convolutions; tests, tools/dev/ab_equal.py") \
    X(GROUP_CONVS,    "SNCAL_GROUP_CONVS",    FLAG, 1,           NET,     "independent convolutions of a module as grouped launches; 0 = one launch each; tests (A/B reference)") \
    X(SUBBATCH,       "SNCAL_SUBBATCH",       INT,  64,          NET,     "frames per sub-batch of a forward (values below 1 are ignored); tests, tools/dev_bench.py, tools/dev/ab_equal.py") \
    X(TT_SMALL_ITEMS, "SNCAL_TT_SMALL_ITEMS", INT,  2,           PLAN,    "two-team launches below this many 8-row items per team take the 96 x 4 x 32 tile (0 = never); tests") \
    X(BBX_MAX_BYTES,  "SNCAL_BBX_MAX_BYTES",  INT,  0xf0000000u, LAUNCH,  "bytes one bblockx3 launch may address; a small limit sends a small batch down the several-launches path; tests") \
    X(HEAD32,         "SNCAL_HEAD32",         INT,  1,           PROCESS, "0 = head.hip in place of head32.hip; tuning aid, set around tools/dev/ab_equal.py runs") \
    X(HEADX3,         "SNCAL_HEADX3",         INT,  1,           PROCESS, "0 = the split head on the generic fp32 kernels in place of headx3.hip; tuning aid, set around tools/dev/ab_equal.py runs") \
    X(HEAD_GM,        "SNCAL_HEAD_GM",        INT,  1,           PROCESS, "0 = head.hip gathers with the VALU, not by MFMA; tuning aid, set around tools/dev/ab_equal.py runs") \
    X(HEAD_STAGE,     "SNCAL_HEAD_STAGE",     INT,  1,           PROCESS, "0 = headx3.hip reads the folded branches' boxes from memory, not through LDS; tuning aid, set around tools/dev/ab_equal.py runs") \
    X(SOLVE_TASKS,    "SNCAL_SOLVE_TASKS",    FLAG, 1,           PROCESS, "one wavefront per (frame, threshold, camera) in the voter; 0 = the four-wave voter_kernel; tests (subprocess A/B reference)") \
    X(SOLVE_WAVE_WGS, "SNCAL_SOLVE_WAVE_WGS", FLAG, 1,           PROCESS, "one-wavefront workgroups in the solve's first pass; 0 = the paired 256-thread calibrate_kernel; tests (subprocess A/B reference)") \
    X(SOLVE_SCHEDULE, "SNCAL_SOLVE_SCHEDULE", STR,  0,           PROCESS, "\"converged\" = the two single-camera entries on the run-to-convergence minimisers, anything else = OpenCV's schedule; include/sncal.h") \
    X(PROFILE_DETAIL, "SNCAL_PROFILE_DETAIL", FLAG, 0,           PROCESS, "one profile row per layer shape / two-team launch kind (was: on by presence, now =0 means off); tuning aid") \
    X(ABLATE,         "SNCAL_ABLATE",         INT,  0,           PROCESS, "ConvParams::ablate (conv.hpp), timing only, results invalid; tuning aid") \
    X(TT_ABLATE,      "SNCAL_TT_ABLATE",      INT,  0,           PROCESS, "TTParams::ablate (conv_tt.hpp), timing only, results invalid; tuning aid, tools/dev/r6") \
    X(BB_DBG,         "SNCAL_BB_DBG",         INT,  0,           PROCESS, "BBlockParams::dbg (bblock.hpp), timing only; tuning aid") \
    X(BBX_DBG,        "SNCAL_BBX_DBG",        INT,  0,           PROCESS, "BBlockX3Params::dbg (bblockx3.hpp), timing only, results invalid; tuning aid") \
    X(BBX_RUNS,       "SNCAL_BBX_RUNS",       INT,  8,           PROCESS, "longest run of tiles a bblockx3 workgroup takes with one ticket (at least 1; bblockx3.hip's RUN_MAX); tuning aid") \
    X(CONV_TRACE,     "SNCAL_CONV_TRACE",     STR,  0,           PROCESS, "layer name: phase stamps of that layer's last generic launch go to conv_trace.bin; tools/conv_trace.py") \
    X(TT_TRACE,       "SNCAL_TT_TRACE",       STR,  0,           PROCESS, "file: per-team phase stamps of the last two-team launch with 3 members; tools/tt_trace.py, tools/dev/tt_trace_run.py") \
    X(TT_TRACE_CFG64, "SNCAL_TT_TRACE_CFG64", FLAG, 0,           PROCESS, "SNCAL_TT_TRACE follows the launches of the 64-channel tile instead; tools/dev/tt_trace_run.py") \
    X(BB_TRACE,       "SNCAL_BB_TRACE",       STR,  0,           PROCESS, "file: phase stamps of the last bblock48 launch; tools/bb_trace.py, tools/dev/bb_trace_run.py") \
    X(BBX_TRACE,      "SNCAL_BBX_TRACE",      STR,  0,           PROCESS, "file: phase stamps of the last bblockx3 launch; tools/bbx_trace.py, tools/dev/bbx_trace_run.py") \
    X(HEAD_TRACE,     "SNCAL_HEAD_TRACE",     STR,  0,           PROCESS, "file: phase stamps of the last head32 / headx3 launch; tools/head_trace.py, tools/dev/head_trace_run.py")

enum EnvId {
#define SNCAL_ENV_ID(id, name, kind, dflt, life, what) ENV_##id,
    SNCAL_ENV_TABLE(SNCAL_ENV_ID)
#undef SNCAL_ENV_ID
    ENV_COUNT
};
bool env_flag(EnvId id);
long long env_int(EnvId id);
const char* env_str(EnvId id);

}  // namespace sncal
