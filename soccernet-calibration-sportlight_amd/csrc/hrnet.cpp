// HRNet plan executor and the sncal_hrnet_* C ABI: the launches of a forward, taps, profiling events, forward_impl, the entry points.
// The plan itself -- op graph, packed weights, workspace layout, launch schedule -- is made by the other host units (hrnet_net.hpp).
#include "hrnet_net.hpp"

extern "C" int sncal_heatmap_decode(const float*, int, int, int, int, int, int, float*, void*);

using namespace sncal;

namespace {

// ---- the launches ---------------------------------------------------------------------------------------------------
struct Call {                    // what one sub-batch of a forward call hands the launches
    int b0, sb, img_h, img_w;
    char* ws;
    const float* x;              // the frames: fp32 NCHW or u8 HWC
    const unsigned char* x8;
    float* heat;                 // the caller's heatmap, or the heat tensor's workspace slot
    float* kpts;                 // this sub-batch's keypoints, or null
    DecodeAt dec;                // where the decode runs in this call
    hipStream_t stream;
};

// parameters of one convolution op on the generic kernel
void conv_params(const sncal_hrnet& net, const Op& op, int sb, char* ws, const Member& m, ConvParams& p) {
    const ConvLayer& L = net.layers[op.conv];
    const Tensor& ti = net.tensors[op.in];
    const Tensor& to = net.tensors[op.out];
    memset(&p, 0, sizeof(p));
    p.range = net.d_range;
    p.in = ws + ti.offset;
    p.out = m.out.dense ? ws + to.offset : nullptr;
    p.out_twin = m.out.twin ? ws + net.tensors[to.twin].offset : nullptr;
    p.res = op.res >= 0 ? ws + net.tensors[op.res].offset : nullptr;
    p.w = L.packed[PK_GENERIC].p; p.w_bytes = (unsigned)L.packed[PK_GENERIC].bytes; p.bias = L.d_bias;
    p.N = sb; p.Hin = ti.H; p.Win = ti.W; p.Cin = ti.C;
    p.Hout = to.H; p.Wout = to.W; p.cout_frags = L.cout_frags; p.cout = L.cout;
    p.out_cstride = to.C; p.out_coff = op.out_coff;
    p.cin_chunks = L.chunks; p.relu = op.relu ? 1 : 0; p.out_f32 = op.out_f32 ? 1 : 0;
    p.twf = m.twf;
    p.twf_log2 = 0;
    while ((1 << p.twf_log2) < m.twf) ++p.twf_log2;
    p.halo_w_magic = 0xFFFFFFFFu / (unsigned)((16 * m.twf - 1) * L.stride + L.k) + 1u;
    p.tiles_x = m.tiles_x; p.tiles_y = m.tiles_y;
    p.epi_lds = m.epi_lds ? 1 : 0;
    p.ablate = env_int(ENV_ABLATE);
    p.nblk = L.nblk;
    p.n_work = (unsigned)(p.tiles_x * p.tiles_y * sb * L.nblk);
    p.per_xcd = (p.n_work + 7) / 8;
    p.nblk_magic = conv_magic((unsigned)L.nblk); p.tiles_x_magic = conv_magic((unsigned)p.tiles_x); p.tiles_y_magic = conv_magic((unsigned)p.tiles_y);
}

void tt_member(const sncal_hrnet& net, const Op& op, const Member& mem, int sb, char* ws, TTMember& m) {
    const ConvLayer& L = net.layers[op.conv];
    const Tensor& ti = net.tensors[op.in];
    const Tensor& to = net.tensors[op.out];
    memset(&m, 0, sizeof(m));
    m.in = ws + ti.offset; m.out = mem.out.dense ? ws + to.offset : nullptr; m.res = op.res >= 0 ? ws + net.tensors[op.res].offset : nullptr;
    m.out8 = mem.out.twin ? ws + net.tensors[to.twin].offset : nullptr;
    m.w = L.packed[PK_TT].p; m.w_bytes = (unsigned)L.packed[PK_TT].bytes; m.bias = L.d_bias;
    m.N = sb; m.H = ti.H; m.W = ti.W; m.Cin = L.cin; m.chunks = tt_chunks(L.cin);
    m.cout = L.cout; m.out_cstride = to.C; m.out_coff = op.out_coff; m.relu = op.relu ? 1 : 0;
    m.in_bytes = (unsigned)((size_t)sb * ti.H * ti.W * ti.C * 2);
    m.hp1_magic = 0xFFFFFFFFu / (unsigned)(ti.H + 1) + 1u;
    if (L.x3_on) {           // bf16x3: split twin in (a bf16 tensor of 2 C pseudo-channels), 16-channel stages, hi / lo weights, fp32 out
        m.in = ws + net.tensors[ti.twin].offset;
        m.in_bytes = (unsigned)((size_t)sb * ti.H * ti.W * ti.C * 4);
        m.Cin = 2 * L.cin;
        m.chunks = ttx3_chunks(L.cin);
        m.w = L.packed[PK_TT_X3].p; m.w_bytes = (unsigned)L.packed[PK_TT_X3].bytes;
        if (op.res_twin) { m.res = ws + net.tensors[net.tensors[op.res].twin].offset; m.res_split = 1; }
    }
    if (L.fp8_on) {          // C5: e4m3 twin in, 64-channel stages, e4m3 weights
        m.in = ws + net.tensors[ti.twin].offset;
        m.in_bytes = (unsigned)((size_t)sb * ti.H * ti.W * ti.C);
        m.chunks = tt8_chunks(L.cin);
        m.w = L.packed[PK_TT_FP8].p; m.w_bytes = (unsigned)L.packed[PK_TT_FP8].bytes;
        m.oscale = L.d_oscale;
        m.out8_inv_scale = mem.out.twin && to.scale > 0.f ? 1.0f / to.scale : 1.0f;
    }
}

// The work lists of a two-team launch (tt_plan_items, conv_tt.hpp) on the device: static per layout, uploaded by the first launch.
int tt_build_plan(const sncal_hrnet& net, const TTMember* mem, int n, TTPlanDev& out, hipStream_t stream) {
    const TTPlan plan = tt_plan_items(mem, n, out.cfg, net.n_cus);
    SNCAL_CHECK_HIP(hipMalloc((void**)&out.items, plan.items.size() * sizeof(TTItem)));
    SNCAL_CHECK_HIP(hipMalloc((void**)&out.first, sizeof plan.first));
    // on the forward's OWN stream, then a wait for that stream only: a plain hipMemcpy runs on the legacy null stream, which synchronises with
    // the pipeline's CU-masked (blocking) solve streams -- a new layout (the tail batch of a directory) then waited for every solve in flight
    SNCAL_CHECK_HIP(hipMemcpyAsync(out.items, plan.items.data(), plan.items.size() * sizeof(TTItem), hipMemcpyHostToDevice, stream));
    SNCAL_CHECK_HIP(hipMemcpyAsync(out.first, plan.first, sizeof plan.first, hipMemcpyHostToDevice, stream));
    SNCAL_CHECK_HIP(hipStreamSynchronize(stream));       // (the host plan dies here; once per layout)
    out.n_wgs = net.n_cus;
    out.lazy = plan.lazy;
    return SNCAL_OK;
}

int run_input(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Tensor& t = net.tensors[net.ops[e.op].out];
    if (c.x8) return launch_u8hwc_to_nhwc(net.dtype, c.x8 + (size_t)c.b0 * 3 * t.H * t.W, c.ws + t.offset, c.sb, t.H, t.W, c.stream);
    return launch_nchw_to_nhwc(net.dtype, c.x + (size_t)c.b0 * 3 * t.H * t.W, c.ws + t.offset, c.sb, 3, t.H, t.W, c.stream, net.d_range);
}

int run_conv(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& op = net.ops[e.op];
    ConvParams p;
    conv_params(net, op, c.sb, c.ws, e.m[0], p);
    // tuning aid: SNCAL_CONV_TRACE=<layer name> dumps per-workgroup phase timestamps of that layer's last launch to conv_trace.bin
    const char* trace_name = env_str(ENV_CONV_TRACE);
    const bool traced = trace_name && net.layers[op.conv].name == trace_name;
    TraceScope trace(traced ? "conv_trace.bin" : nullptr, (size_t)8 * ((p.n_work + 7) / 8) * 16, c.stream);
    p.trace = trace.words;
    e.m[0].v->launch(p, dim3(8 * p.per_xcd), e.m[0].lds, c.stream);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

// the members on the two-team kernel (independent, all eligible, all bf16 or all fp8)
int run_tt(sncal_hrnet& net, Launch& e, const Call& c) {
    const Op* ops = &net.ops[e.op];
    const int n = e.n, sb = c.sb;
    hipStream_t stream = c.stream;
    TTParams tp;
    memset(&tp, 0, sizeof(tp));
    tp.range = net.d_range;
    const bool fp8 = net.layers[ops[0].conv].fp8_on, x3 = net.layers[ops[0].conv].x3_on;
    for (int i = 0; i < n; ++i) {
        LaunchEventsHold hold;       // the profiling event pair belongs to the convolution launch, not to the calibration / quantisation helpers in front of it
        const Tensor& ti = net.tensors[ops[i].in];
        if (net.calibrating && ti.twin >= 0) {        // C5 calibration: max |x| of every candidate input tensor
            const int rc = launch_absmax_bf16(c.ws + ti.offset, (size_t)sb * ti.H * ti.W * ti.C, net.d_amax + ops[i].in, stream);
            if (rc) return rc;
        }
        int rc = SNCAL_OK;
        switch (e.m[i].prep) {       // the input's twin, where no producer wrote it
            case PREP_NONE: break;
            case PREP_SPLIT_F32: rc = launch_split_f32(c.ws + ti.offset, c.ws + net.tensors[ti.twin].offset, (size_t)sb * ti.H * ti.W * ti.C, stream, net.d_range); break;
            case PREP_QUANT_FP8: rc = launch_quantize_fp8(c.ws + ti.offset, c.ws + net.tensors[ti.twin].offset, (size_t)sb * ti.H * ti.W * ti.C, ti.scale, stream); break;
        }
        if (rc) return rc;
        tt_member(net, ops[i], e.m[i], sb, c.ws, tp.m[i]);
    }
    if (!e.plan.n_wgs) {       // static per layout: uploaded by the first launch
        const int rc = tt_build_plan(net, tp.m, n, e.plan, stream);
        if (rc) return rc;
    }
    tp.items = e.plan.items; tp.xcd_first = e.plan.first; tp.lazy = e.plan.lazy;
    tp.queue = net.d_tickets + TICKET_TT;
    // tuning aid: SNCAL_TT_TRACE=<file> dumps the per-team phase timestamps of the LAST launch with 3 members
    // (SNCAL_TT_TRACE_CFG64=1: of the last launch of the 64-channel tile instead)
    const char* trace_file = env_str(ENV_TT_TRACE);
    const bool traced = trace_file && (env_flag(ENV_TT_TRACE_CFG64) ? e.plan.cfg == TT_TILE_64x12 : n == 3);
    TraceScope trace(traced ? trace_file : nullptr, (size_t)e.plan.n_wgs * 2 * 256, stream);
    tp.trace = trace.words;
    tp.ablate = env_int(ENV_TT_ABLATE);
    const int rc = launch_conv_tt(tp, e.plan.n_wgs, fp8 ? 1 : x3 ? 2 : 0, stream, e.plan.cfg);
    if (rc) return rc;
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

// the members as one grouped launch of their common generic variant
int run_group(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op* ops = &net.ops[e.op];
    const int n = e.n;
    ConvGroupParams gp;
    memset(&gp, 0, sizeof(gp));
    size_t lds = 0;
    ConvParams mp[3];
    double cost[3];
    for (int i = 0; i < n; ++i) {
        conv_params(net, ops[i], c.sb, c.ws, e.m[i], mp[i]);
        lds = std::max(lds, e.m[i].lds);
        cost[i] = (double)net.layers[ops[i].conv].chunks;            // K-chunks per work item
    }
    int order[3] = {0, 1, 2};
    std::sort(order, order + n, [&](int a, int b) { return cost[a] > cost[b]; });      // longest items first
    unsigned blocks = 0;
    for (int i = 0; i < n; ++i) {
        gp.p[i] = mp[order[i]];
        gp.per_xcd[i] = (gp.p[i].n_work + 7) / 8;
        blocks += gp.per_xcd[i];
    }
    gp.n = n;
    e.m[0].v->launch_group(gp, dim3(8 * blocks), lds, c.stream);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

// the chain-starting stride-2 convolutions of one input tensor: one launch, tile-major (conv.hpp)
int run_shared_s2(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op* ops = &net.ops[e.op];
    const int n = e.n;
    ConvSharedParams sp;
    memset(&sp, 0, sizeof(sp));
    size_t lds = 0;
    unsigned ipt = 0;
    for (int i = 0; i < n; ++i) {
        conv_params(net, ops[i], c.sb, c.ws, e.m[i], sp.p[i]);
        sp.mi[i] = e.m[i].v->mi;
        sp.first[i] = ipt;
        ipt += (unsigned)sp.p[i].nblk;
        lds = std::max(lds, e.m[i].lds);
    }
    for (int i = n; i < 4; ++i) sp.first[i] = ipt;
    sp.n = n;
    sp.tiles = (unsigned)(sp.p[0].tiles_x * sp.p[0].tiles_y * c.sb);
    sp.tiles_per_xcd = (sp.tiles + 7) / 8;
    launch_conv_shared_s2_x3(sp, 8u * sp.tiles_per_xcd * ipt, lds, c.stream);
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

// layer1's seam (a = conv3 of block b, its output read by b = conv1 of block b + 1) or block 0's tail (a = downsample branch, b = conv3)
int run_bneck(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& a = net.ops[e.op];
    const Op& b = net.ops[e.op + 1];
    const bool tail = e.kind == LK_BNECK_TAIL;
    const Op& conv3 = tail ? b : a;
    const Tensor& t_y = net.tensors[conv3.out];
    BneckPairParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.range = net.d_range;
    bp.h2 = reinterpret_cast<const float*>(c.ws + net.tensors[conv3.in].offset);
    bp.y = reinterpret_cast<float*>(c.ws + t_y.offset);
    bp.w3 = net.layers[conv3.conv].packed[PK_BNP].p; bp.b3 = net.layers[conv3.conv].d_bias;
    if (tail) {
        bp.x0 = reinterpret_cast<const float*>(c.ws + net.tensors[a.in].offset);
        bp.wds = net.layers[a.conv].packed[PK_BNP].p; bp.bds = net.layers[a.conv].d_bias;
    } else {
        bp.res = reinterpret_cast<const float*>(c.ws + net.tensors[a.res].offset);
        bp.h1 = reinterpret_cast<float*>(c.ws + net.tensors[b.out].offset);
        bp.w1 = net.layers[b.conv].packed[PK_BNP].p; bp.b1 = net.layers[b.conv].d_bias;
    }
    bp.P = (long long)c.sb * t_y.H * t_y.W;
    bp.ticket = net.d_tickets + TICKET_SEAM;
    return launch_bneck_pair_x3(bp, net.n_cus, c.stream);
}

int run_bblockx3(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& a = net.ops[e.op];
    const Op& b = net.ops[e.op + 1];
    const Tensor& ti = net.tensors[a.in];
    const Tensor& to = net.tensors[b.out];
    if (e.m[0].prep == PREP_SPLIT_F32) {         // (a helper in front of the launch: not what the profiling events time)
        LaunchEventsHold hold;
        const int rc = launch_split_f32(c.ws + ti.offset, c.ws + net.tensors[ti.twin].offset, (size_t)c.sb * ti.H * ti.W * ti.C, c.stream, net.d_range);
        if (rc) return rc;
    }
    BBlockX3Params bp;
    memset(&bp, 0, sizeof(bp));
    bp.range = net.d_range;
    bp.x = c.ws + net.tensors[ti.twin].offset;
    bp.out_twin = e.m[1].out.twin ? c.ws + net.tensors[to.twin].offset : nullptr;
    bp.out = e.m[1].out.dense ? reinterpret_cast<float*>(c.ws + to.offset) : nullptr;
    bp.w1 = net.layers[a.conv].packed[PK_BBX3].p; bp.b1 = net.layers[a.conv].d_bias;
    bp.w2 = net.layers[b.conv].packed[PK_BBX3].p; bp.b2 = net.layers[b.conv].d_bias;
    bp.N = c.sb; bp.H = ti.H; bp.W = ti.W; bp.out_cstride = to.C; bp.out_coff = b.out_coff;
    bp.ticket = net.d_tickets + TICKET_BBX3;
    return launch_bblockx3(bp, net.n_cus, c.stream);
}

int run_bblock48(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& a = net.ops[e.op];
    const Op& b = net.ops[e.op + 1];
    const Tensor& ti = net.tensors[a.in];
    BBlockParams bp;
    bp.x = c.ws + ti.offset; bp.out = c.ws + net.tensors[b.out].offset;
    bp.w1 = net.layers[a.conv].packed[PK_GENERIC].p; bp.b1 = net.layers[a.conv].d_bias;
    bp.w2 = net.layers[b.conv].packed[PK_GENERIC].p; bp.b2 = net.layers[b.conv].d_bias;
    bp.N = c.sb; bp.H = ti.H; bp.W = ti.W; bp.tiles_x = bp.tiles_y = 0; bp.trace = nullptr;
    bp.ticket = net.d_tickets + TICKET_BB48;
    return launch_bblock48(bp, net.n_cus, c.stream);
}

int run_upadd(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& op = net.ops[e.op];
    const Tensor& to = net.tensors[op.out];
    UpsampleAddParams p;
    memset(&p, 0, sizeof(p));
    p.range = net.d_range;
    p.base = op.base >= 0 ? c.ws + net.tensors[op.base].offset : nullptr;
    p.nsrc = op.nsrc;
    int C0 = to.C;
    for (int s = 0; s < op.nsrc; ++s) {
        const Tensor& ts = net.tensors[op.srcs[s]];
        p.src[s] = c.ws + ts.offset; p.Hs[s] = ts.H; p.Ws[s] = ts.W;
        p.sy[s] = align_corners_ratio(ts.H, to.H);
        p.sx[s] = align_corners_ratio(ts.W, to.W);
        C0 = ts.C;
    }
    p.out = e.m[0].out.dense ? c.ws + to.offset : nullptr;
    p.out_twin = e.m[0].out.twin ? c.ws + net.tensors[to.twin].offset : nullptr;
    p.N = c.sb; p.H = to.H; p.W = to.W; p.C = C0;
    p.out_cstride = to.C; p.out_coff = op.out_coff; p.relu = op.relu ? 1 : 0;
    return launch_upsample_add(net.dtype, p, c.stream);
}

int run_head(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Op& op = net.ops[e.op];
    const Tensor& to = net.tensors[op.out];
    HeadX4Params hp4;
    HeadParams& hp = hp4.h;
    if (op.head_direct < 0) {      // upscale 4: every source is interpolated
        headx4_params(net, op, c.sb, hp4);
        for (int f = 0; f < op.head_nfold; ++f) hp4.fold[f] = c.ws + net.tensors[op.head_fold[f]].offset;
    } else {
        head_params(net, op, c.sb, hp);
        hp.direct = c.ws + net.tensors[op.head_direct].offset;
        for (int s2 = 0; s2 < op.head_nfold; ++s2) hp.fold[s2] = c.ws + net.tensors[op.head_fold[s2]].offset;
    }
    for (int s2 = 0; s2 < op.head_nsrc; ++s2) hp.src[s2] = c.ws + net.tensors[op.head_src[s2]].offset;
    hp.logits = reinterpret_cast<float*>(c.ws + to.offset);
    if (c.dec == DEC_HEAD) {      // log-softmax and the decode's partial maxima in place of the logits
        int rp, cp;
        head32_decode_parts(to.H, to.W, &rp, &cp);
        hp.dec_row = hp.logits; hp.dec_col = hp.logits + (size_t)c.sb * (net.desc.num_classes - 1) * to.H * rp; hp.dec_C = net.desc.num_classes;
    }
    if (op.head_direct < 0) {      // (the layout chose this head by headx4_fits; the rest of headx4_applies holds for every plan it packs)
        if (!net.x3 || !launch_headx4(hp4, c.stream)) { set_error("upscale-4 head: configuration not served by headx4 (set SNCAL_FUSED_HEAD=0)"); return SNCAL_ERR_STATE; }
        SNCAL_CHECK_LAUNCH();
        return SNCAL_OK;
    }
    if (!net.x3) return launch_head_fused(hp, net.head_m2, c.stream);
    if (!launch_headx3(hp, c.stream)) { set_error("fp16x3 head: configuration not served by headx3 (set SNCAL_HEADX3=0)"); return SNCAL_ERR_STATE; }
    SNCAL_CHECK_LAUNCH();
    return SNCAL_OK;
}

int run_tail(const sncal_hrnet& net, const Launch& e, const Call& c) {
    const Tensor& tl = net.tensors[net.ops[e.op].in];
    const int C = net.desc.num_classes;
    if (c.dec == DEC_HEAD) {      // the head already holds log-softmax + the tiles' maxima: the decode's second half only
        int rp, cp;
        head32_decode_parts(tl.H, tl.W, &rp, &cp);
        const float* parts = reinterpret_cast<const float*>(c.ws + tl.offset);        // the logits tensor's slot holds them
        return launch_kp_finish(parts, rp, parts + (size_t)c.sb * (C - 1) * tl.H * rp, cp, C, c.sb, tl.H, tl.W, c.img_h, c.img_w, c.kpts, c.stream);
    }
    if (c.dec == DEC_TAIL)
        return launch_logsoftmax_decode(reinterpret_cast<const float*>(c.ws + tl.offset), tl.C, C, c.sb, tl.H, tl.W, c.img_h, c.img_w, c.heat, c.kpts, c.stream);
    return launch_softmax_nchw(reinterpret_cast<const float*>(c.ws + tl.offset), tl.C, C, (size_t)c.sb * tl.H * tl.W, (size_t)tl.H * tl.W,
                               net.desc.head_softmax ? 0 : 1, c.heat, c.stream);
}

int run_decode(const sncal_hrnet& net, const Call& c) {
    if (!c.kpts || c.dec != DEC_NONE) return SNCAL_OK;         // no keypoints wanted, or decoded already
    const Tensor& th = net.tensors[net.t_heat];
    return sncal_heatmap_decode(c.heat, c.sb, net.desc.num_classes, th.H, th.W, c.img_h, c.img_w, c.kpts, (void*)c.stream);
}

hipEvent_t next_event(sncal_hrnet& net) {
    if (net.events_used == net.event_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        net.event_pool.push_back(e);
    }
    return net.event_pool[net.events_used++];
}

// test instrumentation (sncal_hrnet_plan_tap): copies of the tensors tapped at the ops a launch covered, first sub-batch only, stream-ordered
int run_taps(const sncal_hrnet& net, const Launch& e, const Call& c) {
    if (net.taps.empty() || c.b0 != 0) return SNCAL_OK;
    for (int oi = e.op; oi < e.op + e.n; ++oi)
        for (const sncal_hrnet::Tap& tp : net.taps) {
            if (tp.op != oi) continue;
            const Tensor& tt = net.tensors[tp.tensor];
            if (tt.first < 0) { set_error("sncal_hrnet_plan_tap: tensor %d is not allocated at this layout", tp.tensor); return SNCAL_ERR_STATE; }
            const void* src = tt.external_heat ? (const void*)c.heat : (const void*)(c.ws + tt.offset);
            SNCAL_CHECK_HIP(hipMemcpyAsync(tp.dst, src, tensor_bytes(net, tt, c.sb), hipMemcpyDeviceToDevice, c.stream));
        }
    return SNCAL_OK;
}

// Every forward starts from zeroed ticket words on ITS stream (256 bytes): the kernels re-arm the words themselves, but a launch that
// failed or was torn down half way (device reset by another client, a killed process sharing nothing but the driver) must not leave the
// next forward a counter that skips or repeats work.  A network handle is single-stream: forwards of ONE handle issued on two streams
// at once would share these words (include/sncal.h says so); use one handle per stream (the weights are small against 288 GB).
int rearm_tickets(sncal_hrnet* net, hipStream_t stream) {
    if (!net->d_tickets) SNCAL_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&net->d_tickets), TICKET_WORDS * sizeof(unsigned)));
    SNCAL_CHECK_HIP(hipMemsetAsync(net->d_tickets, 0, TICKET_WORDS * sizeof(unsigned), stream));
    return SNCAL_OK;
}

int forward_impl(sncal_hrnet* net, const float* d_x, const unsigned char* d_x8, int B, int H, int W, float* d_heat,
                        float* d_kpts, int img_h, int img_w, void* d_ws, size_t ws_bytes, void* stream_) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_forward: null net");
    if (!net->finalized) { set_error("sncal_hrnet_forward: weights not finalized"); return SNCAL_ERR_STATE; }
    if (net->fp8 && !net->fp8_calibrated && !net->calibrating) { set_error("sncal_hrnet_forward: fp8 network without calibration (sncal_hrnet_calibrate_fp8)"); return SNCAL_ERR_STATE; }
    SNCAL_CHECK_ARG(B >= 0 && H >= 32 && W >= 32, "sncal_hrnet_forward: bad shape B=%d H=%d W=%d", B, H, W);
    if (B == 0) return SNCAL_OK;
    SNCAL_CHECK_ARG((d_x || d_x8) && d_ws, "sncal_hrnet_forward: null input / workspace");
    SNCAL_CHECK_ARG(d_heat || d_kpts, "sncal_hrnet_forward: need d_heat or d_kpts");
    SNCAL_CHECK_ARG(!(d_kpts && net->desc.head_softmax), "sncal_hrnet_forward: keypoint decode needs a log-softmax head");
    hipStream_t stream = as_stream(stream_);
    const int SB = sub_batch(*net, B, H, W);
    int rc = layout(*net, SB, H, W);
    if (rc) return rc;
    if (ws_bytes < net->lay_bytes) { set_error("workspace too small: %zu < %zu", ws_bytes, net->lay_bytes); return SNCAL_ERR_WORKSPACE; }
    char* ws = reinterpret_cast<char*>(d_ws);
    const Tensor& th = net->tensors[net->t_heat];
    const int C = net->desc.num_classes;
    rc = rearm_tickets(net, stream);
    if (rc) return rc;
    if (net->op_label.size() != net->ops.size()) net->op_label.assign(net->ops.size(), std::string());
    for (int b0 = 0; b0 < B; b0 += SB) {
        const int sb = std::min(SB, B - b0);
        Schedule* s = nullptr;
        rc = schedule_for(*net, sb, &s);
        if (rc) return rc;
        Call c;
        c.b0 = b0; c.sb = sb; c.ws = ws; c.x = d_x; c.x8 = d_x8;
        c.heat = d_heat ? d_heat + (size_t)b0 * C * th.H * th.W : reinterpret_cast<float*>(ws + th.offset);
        c.kpts = d_kpts ? d_kpts + (size_t)b0 * (C - 1) * 3 : nullptr;
        c.img_h = img_h; c.img_w = img_w;
        c.dec = !d_heat && d_kpts ? s->dec : DEC_NONE;          // nobody wants the heatmap: the decode runs where the schedule fused it
        c.stream = stream;
        for (Launch& e : s->launches) {
            hipEvent_t ev0 = nullptr, ev1 = nullptr;
            if (net->profiling == 1 || (net->profiling == 2 && net->op_label[e.op] == net->focus)) {
                ev0 = next_event(*net); ev1 = next_event(*net); sncal::launch_events() = sncal::LaunchEvents{ev0, ev1};
            }
            switch (e.kind) {
                case LK_INPUT: rc = run_input(*net, e, c); break;
                case LK_CONV: rc = run_conv(*net, e, c); break;
                case LK_TT: rc = run_tt(*net, e, c); break;
                case LK_GROUP: rc = run_group(*net, e, c); break;
                case LK_SHARED_S2: rc = run_shared_s2(*net, e, c); break;
                case LK_BNECK_TAIL: case LK_BNECK_SEAM: rc = run_bneck(*net, e, c); break;
                case LK_BBLOCKX3: rc = run_bblockx3(*net, e, c); break;
                case LK_BBLOCK48: rc = run_bblock48(*net, e, c); break;
                case LK_UPADD: rc = run_upadd(*net, e, c); break;
                case LK_HEAD: rc = run_head(*net, e, c); break;
                case LK_TAIL: rc = run_tail(*net, e, c); break;
                case LK_DECODE: rc = run_decode(*net, c); break;
            }
            if (rc) return rc;
            rc = run_taps(*net, e, c);
            if (rc) return rc;
            if (net->profiling) {
                sncal::LaunchEvents& le = sncal::launch_events();
                const bool launched = !le.start && !le.stop;          // the launch consumed the pair
                le = sncal::LaunchEvents{};
                if (!launched || !ev0 || !ev1) continue;
                const Prof& pr = e.kind == LK_TAIL && c.dec != DEC_NONE ? e.prof_kp : e.prof;
                if (net->profiling == 1) net->op_label[e.op] = pr.kernel;
                net->intervals.push_back({ev0, ev1, pr.kernel, pr.flops, pr.bytes});
            }
        }
    }
    return SNCAL_OK;
}

}  // namespace

extern "C" int sncal_hrnet_create(const sncal_hrnet_desc* desc, int dtype, sncal_hrnet** out) {
    SNCAL_CHECK_ARG(desc && out, "sncal_hrnet_create: null pointer");
    SNCAL_CHECK_ARG(dtype == SNCAL_F32 || dtype == SNCAL_BF16 || dtype == SNCAL_FP8 || dtype == SNCAL_BF16X3, "sncal_hrnet_create: dtype %d", dtype);
    SNCAL_CHECK_ARG(desc->stem_width == 64, "stem_width must be 64 (layer1 input is hard-coded, hrnet.py:273)");
    SNCAL_CHECK_ARG(desc->num_classes >= 2 && desc->num_classes <= 64, "num_classes %d out of range", desc->num_classes);
    SNCAL_CHECK_ARG(desc->upscale == 1 || desc->upscale == 2 || desc->upscale == 4, "upscale must be 1, 2 or 4");
    for (int s = 0; s < 3; ++s) {
        SNCAL_CHECK_ARG(desc->num_branches[s] == s + 2, "stage%d must have %d branches", s + 2, s + 2);
        SNCAL_CHECK_ARG(desc->num_modules[s] >= 1 && desc->num_blocks[s] >= 1, "stage%d: modules/blocks", s + 2);
        for (int b = 0; b < desc->num_branches[s]; ++b)
            SNCAL_CHECK_ARG(desc->num_channels[s][b] > 0 && desc->num_channels[s][b] % 16 == 0,
                            "stage%d branch %d: width %d must be a multiple of 16", s + 2, b, desc->num_channels[s][b]);
    }
    SNCAL_CHECK_ARG(desc->stage1_blocks >= 1 && desc->stage1_channels % 16 == 0, "stage1 config");
    sncal_hrnet* net = new sncal_hrnet();
    net->desc = *desc;
    net->fp8 = dtype == SNCAL_FP8;            // C5: the bf16 engine with e4m3 arithmetic in the wide 3x3 stride-1 convolutions
    if (net->fp8) dtype = SNCAL_BF16;
    net->x3 = dtype == SNCAL_BF16X3;          // the fp32 engine with split-bf16 3x3 convolutions
    if (net->x3) dtype = SNCAL_F32;
    net->dtype = dtype;
    net->ge = dtype == SNCAL_BF16 ? 8 : 4;
    net->esize = dtype == SNCAL_BF16 ? 2 : 4;
    net->variants = dtype == SNCAL_BF16 ? conv_variants_bf16(&net->nvariants) : net->x3 ? conv_variants_x3(&net->nvariants) : conv_variants_f32(&net->nvariants);
    if (env_int(ENV_SUBBATCH) > 0) net->subbatch = env_int(ENV_SUBBATCH);
    net->fused_enabled = env_flag(ENV_FUSED_HEAD);
    if (!build_graph(*net)) { delete net; return SNCAL_ERR_STATE; }
    *out = net;
    return SNCAL_OK;
}

extern "C" void sncal_hrnet_destroy(sncal_hrnet* net) {
    if (!net) return;
    drop_layout(*net);
    release_weights(*net);
    for (hipEvent_t e : net->event_pool) (void)hipEventDestroy(e);
    if (net->d_tickets) (void)hipFree(net->d_tickets);
    if (net->d_range) (void)hipFree(net->d_range);
    if (net->d_amax) (void)hipFree(net->d_amax);
    delete net;
}

extern "C" int sncal_hrnet_num_convs(const sncal_hrnet* net) { return net ? net->n_public : 0; }

extern "C" int sncal_hrnet_conv_info(const sncal_hrnet* net, int idx, char* name, int name_cap, char* bn_name, int bn_cap,
                                     int* cin, int* cout, int* ksize, int* stride, int* has_bias) {
    SNCAL_CHECK_ARG(net && idx >= 0 && idx < net->n_public, "sncal_hrnet_conv_info: index %d", idx);
    const ConvLayer& L = net->layers[idx];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", L.name.c_str());
    if (bn_name && bn_cap > 0) snprintf(bn_name, bn_cap, "%s", L.bn.c_str());
    if (cin) *cin = L.cin;
    if (cout) *cout = L.cout;
    if (ksize) *ksize = L.k;
    if (stride) *stride = L.stride;
    if (has_bias) *has_bias = L.bias ? 1 : 0;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_set_conv(sncal_hrnet* net, int idx, const float* h_weight, const float* h_scale, const float* h_shift) {
    SNCAL_CHECK_ARG(net && idx >= 0 && idx < net->n_public, "sncal_hrnet_set_conv: index %d", idx);
    SNCAL_CHECK_ARG(h_weight && h_shift, "sncal_hrnet_set_conv: null weights");
    ConvLayer& L = net->layers[idx];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    L.w.assign(h_weight, h_weight + nw);
    L.scale.assign(L.cout, 1.0f);
    if (h_scale) L.scale.assign(h_scale, h_scale + L.cout);
    L.shift.assign(h_shift, h_shift + L.cout);
    L.is_set = true;
    net->finalized = false;
    net->equalize_done = false;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_set_equalize(sncal_hrnet* net, int enable) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_set_equalize: null");
    net->equalize = enable != 0;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_equalize(sncal_hrnet* net, int* moved) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_equalize: null");
    for (int i = 0; i < net->n_public; ++i)
        if (!net->layers[i].is_set || net->layers[i].w.empty()) { set_error("sncal_hrnet_equalize: conv %s has no weights (call it between sncal_hrnet_set_conv and sncal_hrnet_finalize)", net->layers[i].name.c_str()); return SNCAL_ERR_STATE; }
    if (!net->equalize_done) equalize_blocks(*net);
    if (moved) *moved = net->equalized;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_get_conv(const sncal_hrnet* net, int idx, float* h_weight, float* h_scale, float* h_shift) {
    SNCAL_CHECK_ARG(net && idx >= 0 && idx < net->n_public, "sncal_hrnet_get_conv: index %d", idx);
    const ConvLayer& L = net->layers[idx];
    if (!L.is_set || L.w.empty()) { set_error("sncal_hrnet_get_conv: conv %s holds no host weights (they are released by sncal_hrnet_finalize)", L.name.c_str()); return SNCAL_ERR_STATE; }
    if (h_weight) std::copy(L.w.begin(), L.w.end(), h_weight);
    if (h_scale) std::copy(L.scale.begin(), L.scale.end(), h_scale);
    if (h_shift) std::copy(L.shift.begin(), L.shift.end(), h_shift);
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_finalize(sncal_hrnet* net) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_finalize: null");
    if (const int rc = pack_weights(*net)) return rc;
    if (!net->n_cus) {
        int dev = 0, cus = 0;
        SNCAL_CHECK_HIP(hipGetDevice(&dev));
        SNCAL_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        net->n_cus = cus > 0 ? cus : 256;
    }
    if (net->x3 && !net->d_range) {
        SNCAL_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&net->d_range), 2 * sizeof(unsigned)));
        SNCAL_CHECK_HIP(hipMemset(net->d_range, 0, 2 * sizeof(unsigned)));
    }
    net->finalized = true;
    return SNCAL_OK;
}

// The run-time half of the fp16 range guard (the load-time half is x3_range_check): how many wavefronts have split an activation beyond
// +-65504 (x3.hpp: the value was clamped, the results of those forwards are NOT the reference's) and how many workgroups met a NaN /
// infinite input value, since the counters were last cleared.  Synchronises `stream`.  Engines without the clamp report zeros.
extern "C" int sncal_hrnet_range_status(sncal_hrnet* net, unsigned* overflow, unsigned* nonfinite, int clear, void* stream_) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_range_status: null net");
    unsigned h[2] = {0u, 0u};
    if (net->d_range) {
        hipStream_t stream = as_stream(stream_);
        SNCAL_CHECK_HIP(hipMemcpyAsync(h, net->d_range, sizeof(h), hipMemcpyDeviceToHost, stream));
        if (clear) SNCAL_CHECK_HIP(hipMemsetAsync(net->d_range, 0, sizeof(h), stream));
        SNCAL_CHECK_HIP(hipStreamSynchronize(stream));
    }
    if (overflow) *overflow = h[0];
    if (nonfinite) *nonfinite = h[1];
    if (h[0] || h[1]) {
        set_error("fp16x3 engine: %u wavefront(s) split an activation beyond the fp16 range (clamped to +-65504) and %u workgroup(s) met a NaN / infinite "
                  "input value since the last check: these forwards are not the reference's fp32 result -- use dtype fp32 for this checkpoint / input", h[0], h[1]);
        return SNCAL_ERR_RANGE;
    }
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_output_size(const sncal_hrnet* net, int H, int W, int* out_h, int* out_w) {
    SNCAL_CHECK_ARG(net && H >= 32 && W >= 32, "sncal_hrnet_output_size: bad arguments");
    auto half = [](int v) { return (v + 2 - 3) / 2 + 1; };
    const int h4 = half(half(H)), w4 = half(half(W));
    if (out_h) *out_h = h4 * net->desc.upscale;
    if (out_w) *out_w = w4 * net->desc.upscale;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_workspace(const sncal_hrnet* cnet, int B, int H, int W, size_t* bytes) {
    SNCAL_CHECK_ARG(cnet && bytes && B >= 0 && H >= 32 && W >= 32, "sncal_hrnet_workspace: bad arguments");
    sncal_hrnet* net = const_cast<sncal_hrnet*>(cnet);
    const int sb = sub_batch(*net, B, H, W);
    int rc = layout(*net, sb, H, W);
    if (rc) return rc;
    if (net->finalized) {         // the schedule the first forward of this shape would build (host work only): sncal_plan_op.launch
        Schedule* s = nullptr;
        rc = schedule_for(*net, sb, &s);
        if (rc) return rc;
    }
    *bytes = net->lay_bytes;
    return SNCAL_OK;
}


extern "C" int sncal_hrnet_set_fp8_layers(sncal_hrnet* net, const char* spec) {
    SNCAL_CHECK_ARG(net && spec, "sncal_hrnet_set_fp8_layers: null");
    SNCAL_CHECK_ARG(net->fp8, "sncal_hrnet_set_fp8_layers: the network was not created with SNCAL_FP8");
    unsigned stages = 0;
    std::vector<int> widths;
    bool none = false;
    std::string tok;
    const std::string sp = std::string(spec) + ",";
    for (char ch : sp) {
        if (ch != ',') { if (ch != ' ') tok += ch; continue; }
        if (tok.empty()) continue;
        if (tok == "all") { stages = 0; widths.clear(); }
        else if (tok == "none") none = true;
        else if (tok.size() == 6 && tok.compare(0, 5, "stage") == 0 && tok[5] >= '2' && tok[5] <= '4') stages |= 1u << (tok[5] - '0');
        else if (tok.size() >= 2 && tok[0] == 'c' && atoi(tok.c_str() + 1) > 0) widths.push_back(atoi(tok.c_str() + 1));
        else { set_error("sncal_hrnet_set_fp8_layers: token '%s' (use all, none, stage2..stage4, c<width>)", tok.c_str()); return SNCAL_ERR_ARG; }
        tok.clear();
    }
    net->fp8_stages = none ? (1u << 31) : stages;       // bit 31 matches no stage: nothing selected
    net->fp8_widths = widths;
    drop_layout(*net);                                  // twins / lifetimes depend on the selection
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_calibrate_fp8_workspace(sncal_hrnet* net, int B, int H, int W, size_t* bytes) {
    SNCAL_CHECK_ARG(net && bytes && B >= 0 && H >= 32 && W >= 32, "sncal_hrnet_calibrate_fp8_workspace: bad arguments");
    SNCAL_CHECK_ARG(net->fp8, "sncal_hrnet_calibrate_fp8_workspace: the network was not created with SNCAL_FP8");
    net->calibrating = true; drop_layout(*net);         // the layout sncal_hrnet_calibrate_fp8's forward will use
    const int rc = layout(*net, sub_batch(*net, B, H, W), H, W);
    const size_t n = net->lay_bytes;
    net->calibrating = false; drop_layout(*net);
    if (rc) return rc;
    *bytes = n;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_calibrate_fp8(sncal_hrnet* net, const float* d_x, int B, int H, int W, void* d_ws, size_t ws_bytes, void* stream_) {
    SNCAL_CHECK_ARG(net && d_x && d_ws, "sncal_hrnet_calibrate_fp8: null");
    SNCAL_CHECK_ARG(net->fp8, "sncal_hrnet_calibrate_fp8: the network was not created with SNCAL_FP8");
    hipStream_t stream = as_stream(stream_);
    const size_t nt = net->tensors.size();
    if (!net->d_amax) SNCAL_CHECK_HIP(hipMalloc((void**)&net->d_amax, nt * 4));
    SNCAL_CHECK_HIP(hipMemsetAsync(net->d_amax, 0, nt * 4, stream));
    // keypoints into the (unused) head of the workspace would alias activations: decode into a scratch buffer of our own
    float* d_kp = nullptr;
    SNCAL_CHECK_HIP(hipMalloc((void**)&d_kp, (size_t)B * (net->desc.num_classes - 1) * 3 * 4));
    net->calibrating = true; drop_layout(*net);         // set only around the forward: every exit path below sees it cleared
    const int rc = forward_impl(net, d_x, nullptr, B, H, W, nullptr, d_kp, H, W, d_ws, ws_bytes, stream_);
    net->calibrating = false; drop_layout(*net);
    if (rc) { (void)hipFree(d_kp); return rc; }
    std::vector<float> amax(nt);
    SNCAL_CHECK_HIP(hipStreamSynchronize(stream));
    SNCAL_CHECK_HIP(hipMemcpy(amax.data(), net->d_amax, nt * 4, hipMemcpyDeviceToHost));
    (void)hipFree(d_kp);
    for (size_t t = 0; t < nt; ++t) net->tensors[t].scale = amax[t] > 0.f ? amax[t] / 448.f : 1.f;
    // per-layer output scales: (scale of the layer's input tensor) x (weight scale of the channel)
    for (const Op& op : net->ops) {
        if (op.type != OP_CONV) continue;
        ConvLayer& L = net->layers[op.conv];
        if (!L.packed[PK_TT_FP8].p || net->tensors[op.in].twin < 0) continue;
        std::vector<float> os(L.cout);
        for (int co = 0; co < L.cout; ++co) os[co] = net->tensors[op.in].scale * L.wscale[co];
        SNCAL_CHECK_HIP(hipMemcpy(L.d_oscale, os.data(), os.size() * 4, hipMemcpyHostToDevice));
    }
    net->fp8_calibrated = true;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_set_profiling(sncal_hrnet* net, int enable) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_set_profiling: null");
    SNCAL_CHECK_ARG(enable >= 0 && enable <= 2, "sncal_hrnet_set_profiling: mode %d", enable);
    if (enable == 2) {                  // focus = the kernel variant with the largest total in the profile recorded so far
        std::map<std::string, double> tot;
        for (const auto& iv : net->intervals) {
            SNCAL_CHECK_HIP(hipEventSynchronize(iv.e1));
            float ms = 0;
            SNCAL_CHECK_HIP(hipEventElapsedTime(&ms, iv.e0, iv.e1));
            tot[iv.kernel] += ms;
        }
        SNCAL_CHECK_ARG(!tot.empty(), "sncal_hrnet_set_profiling: mode 2 needs a mode-1 profile of at least one forward first");
        net->focus.clear();
        double best = -1;
        for (const auto& kv : tot) if (kv.second > best) { best = kv.second; net->focus = kv.first; }
    }
    net->profiling = enable;
    net->intervals.clear();
    net->events_used = 0;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_get_profile(sncal_hrnet* net, sncal_kernel_stat* out, int cap, int* count) {
    SNCAL_CHECK_ARG(net && count, "sncal_hrnet_get_profile: null");
    std::map<std::string, sncal_kernel_stat> agg;
    for (const auto& iv : net->intervals) {
        SNCAL_CHECK_HIP(hipEventSynchronize(iv.e1));
        float ms = 0;
        SNCAL_CHECK_HIP(hipEventElapsedTime(&ms, iv.e0, iv.e1));
        sncal_kernel_stat& st = agg[iv.kernel];
        if (st.launches == 0) { memset(&st, 0, sizeof(st)); snprintf(st.kernel, sizeof(st.kernel), "%s", iv.kernel.c_str()); }
        st.flops += iv.flops; st.bytes += iv.bytes; st.ms += ms; st.launches += 1;
    }
    *count = (int)agg.size();
    int i = 0;
    for (const auto& kv : agg) { if (out && i < cap) out[i] = kv.second; ++i; }
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_plan_num_ops(const sncal_hrnet* net) { return net ? (int)net->ops.size() : 0; }
extern "C" int sncal_hrnet_plan_num_tensors(const sncal_hrnet* net) { return net ? (int)net->tensors.size() : 0; }

extern "C" int sncal_hrnet_plan_op(const sncal_hrnet* net, int idx, sncal_plan_op* out) {
    SNCAL_CHECK_ARG(net && out && idx >= 0 && idx < (int)net->ops.size(), "sncal_hrnet_plan_op: index %d", idx);
    const Op& op = net->ops[idx];
    memset(out, 0, sizeof(*out));
    out->type = (int)op.type; out->active = op_active(*net, op) ? 1 : 0; out->conv = op.conv;
    out->in = op.in; out->res = op.res; out->out = op.out; out->base = op.base; out->nsrc = op.nsrc;
    for (int i = 0; i < 4; ++i) out->src[i] = op.srcs[i];
    out->head_direct = op.head_direct; out->head_nsrc = op.head_nsrc; out->head_nfold = op.head_nfold;
    for (int i = 0; i < 5; ++i) out->head_src[i] = i < HEAD_MAX_SRC ? op.head_src[i] : -1;
    for (int i = 0; i < 3; ++i) out->head_fold[i] = i < HEADX4_FOLD ? op.head_fold[i] : -1;
    out->relu = op.relu ? 1 : 0; out->out_coff = op.out_coff; out->out_f32 = op.out_f32 ? 1 : 0;
    if (op.conv >= 0) {
        const ConvLayer& L = net->layers[op.conv];
        snprintf(out->name, sizeof(out->name), "%s", L.name.c_str());
        out->cin = L.cin; out->cout = L.cout; out->ksize = L.k; out->stride = L.stride; out->col_off = L.col_off;
        out->fp8 = L.fp8_on ? 1 : L.x3_on ? 2 : (net->x3 && op.type == OP_CONV) ? 3 : 0;
    }
    out->res_twin = op.res_twin ? 1 : 0;
    out->launch = -1;
    for (const Schedule& s : net->schedules) {
        if (s.sb != net->lay_sb) continue;
        for (size_t k = 0; k < s.launches.size(); ++k) {
            const Launch& e = s.launches[k];
            if (idx < e.op || idx >= e.op + e.n) continue;
            const Member& m = e.m[idx - e.op];
            out->launch = (int)k; out->writes_out = m.out.dense ? 1 : 0; out->writes_twin = m.out.twin ? 1 : 0; out->prep_in = (int)m.prep;
        }
    }
    if (idx < (int)net->op_label.size()) snprintf(out->kernel, sizeof(out->kernel), "%s", net->op_label[idx].c_str());
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_plan_tensor(const sncal_hrnet* net, int id, sncal_plan_tensor* out) {
    SNCAL_CHECK_ARG(net && out && id >= 0 && id < (int)net->tensors.size(), "sncal_hrnet_plan_tensor: id %d", id);
    SNCAL_CHECK_ARG(net->lay_sb > 0, "sncal_hrnet_plan_tensor: no layout yet (call sncal_hrnet_workspace or a forward first)");
    const Tensor& t = net->tensors[id];
    memset(out, 0, sizeof(*out));
    out->C = t.C; out->H = t.H; out->W = t.W; out->dtype = t.f32 ? 0 : t.fp8 ? 2 : (net->dtype == SNCAL_BF16 ? 1 : 0);
    out->twin = t.twin; out->alive = t.first >= 0 ? 1 : 0; out->scale = t.scale;
    if (t.fp8)                      // the calibrated scale is kept on the bf16 tensor the twin belongs to
        for (const Tensor& o : net->tensors) if (o.twin == id) out->scale = o.scale;
    out->sub_batch = net->lay_sb;
    out->bytes = tensor_bytes(*net, t, net->lay_sb);
    out->offset = t.first >= 0 ? t.offset : 0; out->first = t.first; out->last = t.first >= 0 ? t.last : -1;
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_plan_tap(sncal_hrnet* net, int op_idx, int tensor_id, void* d_dst) {
    SNCAL_CHECK_ARG(net, "sncal_hrnet_plan_tap: null");
    if (op_idx < 0) { net->taps.clear(); return SNCAL_OK; }
    SNCAL_CHECK_ARG(op_idx < (int)net->ops.size() && tensor_id >= 0 && tensor_id < (int)net->tensors.size() && d_dst,
                    "sncal_hrnet_plan_tap: op %d tensor %d", op_idx, tensor_id);
    net->taps.push_back({op_idx, tensor_id, d_dst});
    return SNCAL_OK;
}

extern "C" int sncal_hrnet_forward(sncal_hrnet* net, const float* d_x, int B, int H, int W, float* d_heat, float* d_kpts,
                                   int img_h, int img_w, void* d_ws, size_t ws_bytes, void* stream_) {
    return forward_impl(net, d_x, nullptr, B, H, W, d_heat, d_kpts, img_h, img_w, d_ws, ws_bytes, stream_);
}

extern "C" int sncal_hrnet_forward_u8(sncal_hrnet* net, const unsigned char* d_x, int B, int H, int W, float* d_heat,
                                      float* d_kpts, int img_h, int img_w, void* d_ws, size_t ws_bytes, void* stream_) {
    return forward_impl(net, nullptr, d_x, B, H, W, d_heat, d_kpts, img_h, img_w, d_ws, ws_bytes, stream_);
}

