// The launch schedule of a sub-batch at the current layout: which kernel runs which ops, decided once per (layout, sub-batch size) by
// the eligibility and fusion predicates below, with each launch's tile choice and profile row.  forward_impl only dispatches on it.
#include "hrnet_net.hpp"

using namespace sncal;

// ---- two-team persistent kernel for the wide 3x3 stride-1 convolutions (conv_tt.hip) --------------------------------
bool sncal::tt_eligible(const sncal_hrnet& net, const Op& op, int sb) {
    if (!net.use_conv_tt || op.type != OP_CONV) return false;
    const ConvLayer& L = net.layers[op.conv];
    const Tensor& ti = net.tensors[op.in];
    const Tensor& to = net.tensors[op.out];
    if (net.x3) {                                   // bf16x3 engine: fp32 tensors, split twin in, fp32 out
        if (net.dtype != SNCAL_F32 || !L.packed[PK_TT_X3].p || ti.C != L.cin || ti.twin < 0 || to.C % 8 || op.out_coff % 8) return false;
        // every whole-tensor byte count the kernel forms (input twin, fp32 output, output twin, residual) stays below 2^31: its epilogue
        // relies on voffset 0x80000000 + soffset being out of range for masked lanes, which only holds for ranges below that
        const size_t in_bytes = (size_t)sb * ti.H * ti.W * ti.C * 4, out_bytes = (size_t)sb * to.H * to.W * to.C * 4;
        const size_t twin_bytes = (size_t)sb * to.H * to.W * L.cout * 4;
        return in_bytes < (1u << 31) && out_bytes < (1u << 31) && twin_bytes < (1u << 31) &&
               L.packed[PK_TT_X3].bytes < (1u << 31);
    }
    if (net.dtype != SNCAL_BF16 || op.out_f32) return false;
    if (!L.packed[PK_TT].p || ti.C != L.cin) return false;                                   // packed at finalize for the eligible shapes
    if (to.C % 8 || op.out_coff % 8) return false;
    const size_t in_bytes = (size_t)sb * ti.H * ti.W * ti.C * 2, out_elems = (size_t)sb * to.H * to.W * to.C;
    return in_bytes < (1u << 31) && out_elems < (1ull << 32) && L.packed[PK_TT].bytes < (1u << 31) && L.packed[PK_TT_FP8].bytes < (1u << 31);
}

namespace {

// does the active op that produced tensor t write its e4m3 / split twin itself?  Asked once per tensor, by twin_table
bool twin_written_by_producer(const sncal_hrnet& net, int t, int sb) {
    const int pi = t >= 0 && t < (int)net.producer.size() ? net.producer[t] : -1;
    if (pi < 0) return false;
    const Op& po = net.ops[pi];
    if (po.type == OP_CONV && net.layers[po.conv].x3_on && tt_eligible(net, po, sb))        // bf16x3: the producer's epilogue writes the split twin
        return po.out_coff == 0 && net.tensors[po.out].C == net.layers[po.conv].cout;     // (dense outputs only)
    if (net.x3 && net.dtype == SNCAL_F32) {
        // bf16x3: the generic split-arithmetic convolution and the fp32 fuse sum write the twin of a dense output in their epilogues
        if (po.type == OP_CONV && !net.layers[po.conv].x3_on && po.out_coff == 0 && !po.out_f32 &&
            net.tensors[po.out].C == net.layers[po.conv].cout && net.layers[po.conv].cout % 16 == 0) return true;
        if (po.type == OP_UPADD && po.out_coff == 0 && net.tensors[po.out].C % 16 == 0) return true;
    }
    return po.type == OP_CONV && net.layers[po.conv].fp8_on && tt_eligible(net, po, sb);
}

// Schedule::twin_by: for every tensor whose twin is alive at this layout, whether its producer's epilogue writes the twin or a helper
// makes it in front of each launch that reads it
void twin_table(const sncal_hrnet& net, int sb, std::vector<TwinBy>& by) {
    by.assign(net.tensors.size(), TW_NONE);
    for (size_t t = 0; t < net.tensors.size(); ++t) {
        const int tw = net.tensors[t].twin;
        if (tw >= 0 && net.tensors[tw].first >= 0) by[t] = twin_written_by_producer(net, (int)t, sb) ? TW_PRODUCER : TW_FRONT;
    }
}

// The forms of op's output that its launch writes.  Split engine: the twin when the table has the producer write it, the fp32 tensor when
// there is no such twin or somebody reads the fp32 form.  e4m3 convolution (two-team kernel only): the twin whenever it is alive, the
// bf16 tensor iff somebody reads it.  Everything else writes the tensor alone.
Forms out_forms(const sncal_hrnet& net, const Schedule& s, const Op& op, LaunchKind kind) {
    if (op.out < 0) return Forms{};
    if (kind == LK_TT && net.layers[op.conv].fp8_on) return Forms{net.need_bf16[op.out] != 0, s.twin_by[op.out] != TW_NONE};
    if (!net.x3) return Forms{};
    const bool twin = s.twin_by[op.out] == TW_PRODUCER;
    return Forms{!twin || net.need_bf16[op.out], twin};
}

// the helper in front of the launch of a reduced-precision convolution whose input twin no producer wrote
Prep prep_in(const sncal_hrnet& net, const Schedule& s, const Op& op) {
    const ConvLayer& L = net.layers[op.conv];
    if (!(L.fp8_on || L.x3_on) || s.twin_by[op.in] != TW_FRONT) return PREP_NONE;
    return L.fp8_on ? PREP_QUANT_FP8 : PREP_SPLIT_F32;
}

bool profile_detail() { return env_flag(ENV_PROFILE_DETAIL); }      // tuning aid: one profile row per layer shape / two-team launch kind

// the generic kernel's variant, tile shape and dynamic LDS size for one convolution op at this layout (no launch)
int choose_conv(const sncal_hrnet& net, const Op& op, int sb, Member& m) {
    const ConvLayer& L = net.layers[op.conv];
    const Tensor& ti = net.tensors[op.in];
    const Tensor& to = net.tensors[op.out];
    // one IMAGE of the input / output tensor is a buffer-descriptor range in the kernel (int byte counts, out-of-range sentinel 0x80000000)
    if ((size_t)ti.H * ti.W * ti.C * 4 >= (1u << 31) || (size_t)to.H * to.W * to.C * 4 >= (1u << 31)) {
        set_error("conv %s: one image of a tensor reaches 2 GB (%dx%dx%d -> %dx%dx%d): unsupported", L.name.c_str(), ti.H, ti.W, ti.C, to.H, to.W, to.C);
        return SNCAL_ERR_UNSUPPORTED;
    }
    // pick NI / tile shape / sub-tiles per weight chunk for this spatial size
    m.v = nullptr;
    m.lds = 0;
    m.twf = 1;
    double best_score = -1;
    const double three_gain = 1.15;     // of a third co-resident workgroup (was a tuning aid)
    for (int v = 0; v < net.nvariants; ++v) {
        const ConvVariant& V = net.variants[v];
        if (V.ks != L.k || V.stride != L.stride || V.mi != L.mi || V.g != L.g) continue;
        const int F = 4 * V.ni;
        const size_t wchunk = (size_t)conv_nks(V.ks, V.g) * V.mi * 1024;
        for (int twf = 1; twf <= F; twf *= 2) {
            if (F % twf) continue;
            const int th = F / twf;
            const size_t lds = conv_stage_bytes(V.ks, V.stride, V.ni, V.mi, V.g, twf);
            if (lds > 160 * 1024 || lds - wchunk > 64 * 1024) continue;   // halo tiles are capped at 64 DMA pieces
            const long ty = (to.H + th - 1) / th, tx = (to.W + 16 * twf - 1) / (16 * twf);
            const double eff = (double)to.H * to.W / ((double)ty * th * tx * 16 * twf);
            const long blocks = ty * tx * sb * L.nblk;
            const int per_cu = (int)std::min<size_t>(conv_resident_wgs(V.ks, V.ni, V.mi, V.g), (160 * 1024) / lds);
            const double fill = std::min(1.0, (double)blocks / (256.0 * per_cu));
            const double reuse = (double)(V.mi * V.ni) / (V.mi + V.ni);       // MFMAs per LDS fragment read
            // exposed staging latency is hidden by co-resident workgroups only (see conv.hpp)
            const double overlap = per_cu >= 3 ? three_gain : per_cu >= 2 ? 1.0 : 0.55;
            const double score = eff * (0.3 + 0.7 * fill) * std::pow(reuse, 0.6) * overlap;
            if (score > best_score + 1e-9) { best_score = score; m.v = &V; m.twf = twf; m.lds = lds; }
        }
    }
    if (!m.v) { set_error("no conv variant for %s (k=%d s=%d mi=%d g=%d)", L.name.c_str(), L.k, L.stride, L.mi, L.g); return SNCAL_ERR_STATE; }
    const int th = 4 * m.v->ni / m.twf;
    m.tiles_x = (to.W + 16 * m.twf - 1) / (16 * m.twf);
    m.tiles_y = (to.H + th - 1) / th;
    {   // LDS-transposed epilogue: the fp32 tile of the 4 waves is staged in the (grown, if that keeps two
        // workgroups per CU) dynamic LDS; bf16: whole 8-channel groups, fp32 / bf16x3 engines (epilogue F): whole 4-channel groups
        const int wgs = conv_resident_wgs(L.k, m.v->ni, L.mi, L.g);
        const size_t need = (size_t)4 * conv_epi_frags(L.k, m.v->ni, L.mi, L.g) * 16 * (L.mi * 16 + 4) * 4;
        const bool shape_ok = net.dtype == SNCAL_BF16 ? (!op.out_f32 && L.cout % 8 == 0 && to.C % 8 == 0 && op.out_coff % 8 == 0)
                                                     : (L.cout % 4 == 0 && to.C % 4 == 0 && op.out_coff % 4 == 0);
        const size_t now_per_cu = std::min<size_t>(wgs, (160 * 1024) / m.lds);
        const bool fits = need <= m.lds || need <= (160 * 1024) / now_per_cu || need <= 52 * 1024;
        m.epi_lds = shape_ok && fits;
        if (m.epi_lds && need > m.lds) m.lds = need;
    }
    return SNCAL_OK;
}

// profile row of one convolution op (a launch of several members sums them; the last one names the row)
Prof conv_prof(const sncal_hrnet& net, const Op& op, int sb, const ConvVariant* v) {
    const ConvLayer& L = net.layers[op.conv];
    const Tensor& ti = net.tensors[op.in];
    const Tensor& to = net.tensors[op.out];
    Prof r;
    r.kernel = fmt("conv<%s,k%d,s%d,NI%d,MI%d,G%d>", net.dtype == SNCAL_BF16 ? "bf16" : net.x3 ? SNCAL_X3_NAME : "f32", L.k, L.stride, v ? v->ni : 0, L.mi, L.g);
    if (profile_detail()) r.kernel += fmt("@%dx%d:%d->%d%s", to.H, to.W, L.cin, L.cout, op.res >= 0 ? "+res" : "");
    const double px = (double)sb * to.H * to.W;
    r.flops = 2.0 * px * L.cout * L.cin * L.k * L.k;
    r.bytes = (double)sb * ti.H * ti.W * ti.C * net.esize + px * L.cout * (op.out_f32 ? 4 : net.esize) * (op.res >= 0 ? 2 : 1) +
              (double)L.cout * L.cin * L.k * L.k * net.esize;
    return r;
}

void add_prof(Prof& sum, const Prof& member) { sum.kernel = member.kernel; sum.flops += member.flops; sum.bytes += member.bytes; }

// Work-list tile of a two-team launch: TT_TILE_96x8, TT_TILE_64x12 (bf16x3, 48-channel branch) or TT_TILE_96x4.  Small launches of the
// split-arithmetic engine (round 5): below two 8-row items per team the launch lasts as long as its longest item while most teams hold short
// ones or nothing -- the 96 x 4 x 32 tile (conv_tt.hip) halves the items instead
TTTile tt_cfg(const sncal_hrnet& net, const Op* ops, int n, int sb) {
    const ConvLayer& L0 = net.layers[ops[0].conv];
    if (!L0.x3_on) return TT_TILE_96x8;
    if (n == 1 && L0.x3_blk == TT_TILES[TT_TILE_64x12].cout_blk) return TT_TILE_64x12;
    const int per_team = env_int(ENV_TT_SMALL_ITEMS);      // (read per plan: tests run both tiles in one process; 0 = never)
    long items = 0;
    for (int i = 0; i < n; ++i) {
        const Tensor& ti = net.tensors[ops[i].in];
        items += tt_grid(sb, ti.H, ti.W, net.layers[ops[i].conv].cout, TT_TILE_96x8).items();
    }
    return items < (long)per_team * 2 * net.n_cus ? TT_TILE_96x4 : TT_TILE_96x8;
}

// ---- the schedule builder: fusion predicates, asked once per (layout, sub-batch size) --------------------------------

// layer1 block 0's tail (bneckx3.hip): op i is the downsample branch, op i + 1 the conv3 that adds it
bool fuses_bneck_tail(const sncal_hrnet& net, const Schedule& s, size_t i) {
    const Op& op = net.ops[i];
    if (!(net.fuse_bneck & 2) || !net.x3 || op.relu || op.res >= 0 || op.out_f32 || op.out_coff != 0 || i + 1 >= net.ops.size() ||
        !net.layers[op.conv].packed[PK_BNP].p || net.layers[op.conv].cout != BNP_WIDE || net.layers[op.conv].x3_on || op.launch_group >= 0) return false;
    const Op& nx = net.ops[i + 1];
    return nx.type == OP_CONV && op_active(net, nx) && nx.res == op.out && nx.relu && !nx.out_f32 && nx.out_coff == 0 && nx.launch_group < 0 &&
           net.layers[nx.conv].packed[PK_BNP].p && net.layers[nx.conv].cout == BNP_WIDE && !net.layers[nx.conv].x3_on &&
           net.tensors[op.in].C == BNP_MID && net.tensors[nx.in].C == BNP_MID && net.tensors[nx.out].C == BNP_WIDE &&
           net.tensors[op.in].H == net.tensors[nx.in].H && net.tensors[op.in].W == net.tensors[nx.in].W &&
           net.tensors[op.out].last_read == (int)i + 1 &&      // nobody else reads the downsample branch
           s.twin_by[nx.out] != TW_PRODUCER;                   // nobody is owed a split twin of the block output
}

// layer1 (bneckx3.hip): conv3 (+ residual, ReLU) of a Bottleneck and conv1 (+ ReLU) of the next one in one pass over the pixels: the
// 256-channel tensor between them is written once (the next residual) and not read back
bool fuses_bneck_seam(const sncal_hrnet& net, const Schedule& s, size_t i) {
    const Op& op = net.ops[i];
    if (!(net.fuse_bneck & 1) || !net.x3 || !op.relu || op.res < 0 || op.out_f32 || op.out_coff != 0 || i + 1 >= net.ops.size() ||
        !net.layers[op.conv].packed[PK_BNP].p || net.layers[op.conv].cout != BNP_WIDE || net.layers[op.conv].x3_on) return false;
    const Op& nx = net.ops[i + 1];
    const Tensor& t_in = net.tensors[op.in];
    const Tensor& t_res = net.tensors[op.res];
    const Tensor& t_y = net.tensors[op.out];
    return nx.type == OP_CONV && op_active(net, nx) && nx.in == op.out && nx.res < 0 && nx.relu && !nx.out_f32 && nx.out_coff == 0 &&
           nx.launch_group < 0 && net.layers[nx.conv].packed[PK_BNP].p && net.layers[nx.conv].cout == BNP_MID && !net.layers[nx.conv].x3_on &&
           t_in.C == BNP_MID && t_res.C == BNP_WIDE && t_y.C == BNP_WIDE && net.tensors[nx.out].C == BNP_MID &&
           t_res.H == t_y.H && t_res.W == t_y.W &&
           s.twin_by[op.out] != TW_PRODUCER && s.twin_by[nx.out] != TW_PRODUCER;      // neither output may owe somebody a split twin (they feed generic kernels)
}

// bf16x3 engine, 48-channel BasicBlock: conv1 -> mid tile in LDS as hi / lo planes -> conv2 + residual (bblockx3.hip); the mid tensor and
// its twin are not written at all
bool fuses_bblockx3(const sncal_hrnet& net, const Schedule& s, size_t i) {
    const int sb = s.sb;
    const Op& op = net.ops[i];
    if (!net.x3 || !op.relu || op.res >= 0 || op.out_f32 || i + 1 >= net.ops.size() || !net.layers[op.conv].x3_on ||
        !net.layers[op.conv].packed[PK_BBX3].p || !tt_eligible(net, op, sb)) return false;
    const Op& nx = net.ops[i + 1];
    return nx.type == OP_CONV && op_active(net, nx) && nx.in == op.out && nx.res == op.in && nx.relu && !nx.out_f32 && op.out_coff == 0 &&
           net.layers[nx.conv].x3_on && net.layers[nx.conv].packed[PK_BBX3].p && tt_eligible(net, nx, sb) && net.tensors[op.in].C == 48 &&
           s.twin_by[op.in] != TW_NONE;
}

// bf16 engine, 48-channel BasicBlock: conv1 + conv2 (+ residual) fused when the next active op is its second convolution and both layers
// carry the (MI = 3, G = 3) packing (bblock.hip)
bool fuses_bblock48(const sncal_hrnet& net, size_t i) {
    const Op& op = net.ops[i];
    if (!net.fuse_bblock || net.dtype != SNCAL_BF16 || !op.relu || op.res >= 0 || op.out_f32 || i + 1 >= net.ops.size()) return false;
    const Op& nx = net.ops[i + 1];
    if (nx.type != OP_CONV || !op_active(net, nx) || nx.in != op.out || nx.res != op.in || !nx.relu || nx.out_f32 || nx.out_coff != 0 || op.out_coff != 0)
        return false;
    auto ok = [](const ConvLayer& L) { return L.k == 3 && L.stride == 1 && L.cin == 48 && L.cout == 48 && L.cin_phys == 48 && L.mi == 3 && L.g == 3 &&
                                              L.chunks == 2 && L.nblk == 1; };
    return ok(net.layers[op.conv]) && ok(net.layers[nx.conv]) && net.tensors[op.in].C == 48 && net.tensors[nx.out].C == 48;
}

// The members [i, i + n) of a launch group (independent convolutions, consecutive ops) as ONE launch when they can share one: all on the
// two-team kernel, the shared-input stride-2 kernel, or one grouped variant of the generic kernel.  Otherwise e stays untouched (e.n == 1)
// and the caller takes the first member alone, then tries the rest again.
int plan_group(const sncal_hrnet& net, size_t i, int n, int sb, Launch& e) {
    if (n < 2 || n > 3) return SNCAL_OK;
    const Op* ops = &net.ops[i];
    bool all_tt = true, any_fp8 = false, all_fp8 = true;
    int couts = 0;
    for (int k = 0; k < n; ++k) {
        const ConvLayer& L = net.layers[ops[k].conv];
        all_tt = all_tt && tt_eligible(net, ops[k], sb) && L.fp8_on == net.layers[ops[0].conv].fp8_on && !(L.x3_on && L.x3_blk != TT_COUT);
        couts += (L.cout + TT_COUT - 1) / TT_COUT * TT_COUT;
        any_fp8 = any_fp8 || L.fp8_on;
        all_fp8 = all_fp8 && L.fp8_on;
    }
    if (any_fp8 && !all_fp8) return SNCAL_OK;     // fp8 and bf16 members (layer selection by width) cannot share one launch
    if (all_tt && couts <= TT_COUT_MAX) {         // (the tables' last 16 floats carry the ticket queue's slots)
        e.kind = LK_TT; e.n = n; e.plan.cfg = tt_cfg(net, ops, n, sb);
        return SNCAL_OK;
    }
    // A member the two-team kernel serves never joins a grouped launch of the GENERIC kernel: a group too wide for the tables (288 + 480
    // = 768 channels) or with a member past the kernel's widths (288 + 480 + 576) is taken apart -- the first member alone, the rest tried
    // again -- so that every eligible layer keeps its kernel.  (Without this the members that happened to pick one generic variant went out
    // as LK_GROUP: 288- and 480-channel layers on the generic kernel in some layouts and on the two-team kernel in others.  No packaged
    // config gets here: their eligible members always fit one two-team launch.)
    for (int k = 0; k < n; ++k)
        if (tt_eligible(net, ops[k], sb)) return SNCAL_OK;
    // the chain-starting stride-2 convolutions of one input tensor (schedule_fuse_section): one launch, tile-major (conv.hpp)
    if (ops[0].shared_in && !net.x3) return SNCAL_OK;        // (the other engines run them one by one)
    Member m[3];
    for (int k = 0; k < n; ++k) {
        const int rc = choose_conv(net, ops[k], sb, m[k]);
        if (rc) return rc;
    }
    if (ops[0].shared_in) {
        for (int k = 0; k < n; ++k) {
            const ConvVariant* v = m[k].v;
            if (ops[k].in != ops[0].in || v->ks != 3 || v->stride != 2 || v->ni != 2 || v->g != 3 || (v->mi != 6 && v->mi != 3) ||
                m[k].tiles_x != m[0].tiles_x || m[k].tiles_y != m[0].tiles_y || m[k].twf != m[0].twf) return SNCAL_OK;
        }
        e.kind = LK_SHARED_S2;
    } else {
        for (int k = 0; k < n; ++k)
            if (m[k].v != m[0].v || !m[k].v->launch_group) return SNCAL_OK;
        e.kind = LK_GROUP;
    }
    e.n = n;
    std::copy(m, m + n, e.m);
    return SNCAL_OK;
}

void profile_launch(const sncal_hrnet& net, const Schedule& s, Launch& e) {
    const Op& op = net.ops[e.op];
    const Op* ops = &op;
    const int sb = s.sb, C = net.desc.num_classes;
    const Tensor& th = net.tensors[net.t_heat];
    Prof& r = e.prof;
    switch (e.kind) {
        case LK_INPUT: {
            const Tensor& t = net.tensors[op.out];
            r = {"nchw_to_nhwc", 0, (double)sb * t.H * t.W * (3 * 4 + net.ge * net.esize)};
            break;
        }
        case LK_CONV: r = conv_prof(net, op, sb, e.m[0].v); break;
        case LK_GROUP: for (int k = 0; k < e.n; ++k) add_prof(r, conv_prof(net, ops[k], sb, e.m[0].v)); break;
        case LK_SHARED_S2: {
            for (int k = 0; k < e.n; ++k) add_prof(r, conv_prof(net, ops[k], sb, e.m[k].v));
            const Tensor& ti = net.tensors[op.in];
            r.bytes -= (double)(e.n - 1) * sb * ti.H * ti.W * ti.C * net.esize;      // the members' common input counts once
            if (!profile_detail()) r.kernel = "conv_shared_s2<" SNCAL_X3_NAME ",k3,NI2,G3>";     // (its own row: not the first member's variant)
            break;
        }
        case LK_TT: {
            for (int k = 0; k < e.n; ++k) add_prof(r, conv_prof(net, ops[k], sb, nullptr));
            const ConvLayer& L0 = net.layers[op.conv];
            r.kernel = fmt("conv_tt<%s,k3,s1,%s>", L0.fp8_on ? "fp8" : L0.x3_on ? SNCAL_X3_NAME : "bf16", TT_TILES[e.plan.cfg].label);
            if (profile_detail()) {      // one profile row per launch kind
                r.kernel += fmt("@%d members%s%s%s", e.n, op.res >= 0 ? "+res" : "", e.m[0].out.dense ? "+f32" : "", e.m[0].out.twin ? "+twin" : "");
            }
            break;
        }
        case LK_BNECK_TAIL: case LK_BNECK_SEAM: {
            const bool tail = e.kind == LK_BNECK_TAIL;
            const Tensor& t_y = net.tensors[ops[tail ? 1 : 0].out];
            const long long P = (long long)sb * t_y.H * t_y.W;
            r.kernel = tail ? "bneck_tail_ds_x3" : "bneck_seam_x3";
            r.flops = 2.0 * 2.0 * (double)P * BNP_MID * BNP_WIDE;
            r.bytes = tail ? (double)P * 4.0 * (BNP_MID + BNP_MID + BNP_WIDE) + 2.0 * BNP_W_BYTES
                           : (double)P * 4.0 * (BNP_MID + BNP_WIDE + BNP_WIDE + BNP_MID) + 2.0 * BNP_W_BYTES;
            break;
        }
        case LK_BBLOCKX3: case LK_BBLOCK48: {
            const Tensor& ti = net.tensors[op.in];
            const double px = (double)sb * ti.H * ti.W;
            r.flops = 2.0 * 2.0 * px * 48 * 48 * 9;
            if (e.kind == LK_BBLOCKX3) { r.kernel = "bblockx3_fused"; r.bytes = px * 48 * 4 * (1.0 + (e.m[1].out.twin ? 1.0 : 0.0) + (e.m[1].out.dense ? 1.0 : 0.0)) + 2.0 * BBX_W_BYTES; }
            else { r.kernel = "bblock48_fused"; r.bytes = 2.0 * px * 48 * 2 + 2.0 * 48 * 48 * 9 * 2; }
            break;
        }
        case LK_UPADD: {
            const Tensor& to = net.tensors[op.out];
            double b = 0;
            for (int s2 = 0; s2 < op.nsrc; ++s2) { const Tensor& ts = net.tensors[op.srcs[s2]]; b += (double)sb * ts.H * ts.W * ts.C * net.esize; }
            const int C0 = op.nsrc ? net.tensors[op.srcs[0]].C : to.C;
            r = {"upsample_add", 0, b + (double)sb * to.H * to.W * C0 * net.esize * (op.base >= 0 ? 2 : 1)};
            break;
        }
        case LK_HEAD: {
            const Tensor& to = net.tensors[op.out];
            const double px = (double)sb * to.H * to.W;
            r.kernel = !net.x3 ? "head_fused" : op.head_direct < 0 ? "headx4_fused" : "headx3_fused";
            r.flops = 2.0 * px * net.head_hp * (net.head_k + net.head_m2 * 16);
            r.bytes = px * ((op.head_direct >= 0 ? net.tensors[op.head_direct].C * 2 : 0) + to.C * 4);
            for (int s2 = 0; s2 < op.head_nsrc; ++s2) { const Tensor& ts = net.tensors[op.head_src[s2]]; r.bytes += (double)sb * ts.H * ts.W * ts.C * 2; }
            for (int s2 = 0; s2 < op.head_nfold; ++s2) { const Tensor& tf = net.tensors[op.head_fold[s2]]; r.bytes += (double)sb * tf.H * tf.W * tf.C * 2; }
            break;
        }
        case LK_TAIL: {
            const Tensor& tl = net.tensors[op.in];
            r = {"softmax_nchw", 0, (double)sb * C * th.H * th.W * 4 * 2};
            e.prof_kp = s.dec == DEC_HEAD ? Prof{"kp_finish", 0, (double)head32_decode_scratch(sb, C, tl.H, tl.W)}
                      : s.dec == DEC_TAIL ? Prof{"logsoftmax_decode_fused", 0, (double)sb * tl.H * tl.W * tl.C * 4} : r;
            break;
        }
        case LK_DECODE: r = {"kp_decode", 0, (double)sb * C * th.H * th.W * 4}; break;
    }
}

// Where the keypoint decode runs when a call wants keypoints and no heatmap: inside the head (head32.hip / headx3.hip: log-softmax and the
// tiles' maxima, the logits tensor's own workspace slot -- alive from the head to the softmax op -- holds the partial maxima, kp_finish
// completes them), else fused with the log-softmax (the (B,C,h,w) tensor is never written; its workspace slot serves as the much smaller
// scratch), else after a plain softmax.
DecodeAt decode_at(const sncal_hrnet& net, const Schedule& s) {
    const int C = net.desc.num_classes, sb = s.sb;
    const Tensor& th = net.tensors[net.t_heat];
    if (net.desc.head_softmax) return DEC_NONE;
    for (const Launch& e : s.launches) {
        const Op& op = net.ops[e.op];
        if (e.kind == LK_HEAD) {
            const Tensor& to = net.tensors[op.out];
            HeadParams hp;
            HeadX4Params hp4;
            bool serves;
            if (op.head_direct < 0) { headx4_params(net, op, sb, hp4); serves = net.x3 && headx4_applies(hp4); }
            else { head_params(net, op, sb, hp); serves = net.x3 ? headx3_applies(hp) : head32_applies(hp); }
            if (C > 32 && C <= 64 && serves &&
                head32_decode_scratch(sb, C, to.H, to.W) <= to.bytes && th.H == to.H && th.W == to.W) return DEC_HEAD;
        }
        if (e.kind == LK_TAIL) {
            const Tensor& tl = net.tensors[op.in];
            if (logsoftmax_decode_scratch(sb, C, tl.H, tl.W) <= (size_t)sb * C * th.H * th.W * sizeof(float)) return DEC_TAIL;
        }
    }
    return DEC_NONE;
}

// The launch schedule of a sub-batch of sb frames at the current layout.  Fusions, in this order of priority: a launch group over the
// remaining consecutive members; layer1's downsample tail, then its seams, then the split-arithmetic BasicBlock, then the bf16 one; else
// the op alone, on the two-team kernel when it is eligible.
int build_schedule(const sncal_hrnet& net, int sb, Schedule& s) {
    s.sb = sb;
    twin_table(net, sb, s.twin_by);
    for (size_t i = 0; i < net.ops.size();) {
        const Op& op = net.ops[i];
        if (!op_active(net, op)) { ++i; continue; }
        Launch e;
        e.op = (int)i;
        switch (op.type) {
            case OP_INPUT: e.kind = LK_INPUT; break;
            case OP_CONV: {
                int n = 0;
                if (op.launch_group >= 0)
                    while (i + n < net.ops.size() && net.ops[i + n].launch_group == op.launch_group && net.ops[i + n].type == OP_CONV &&
                           op_active(net, net.ops[i + n])) ++n;
                int rc = plan_group(net, i, n, sb, e);
                if (rc) return rc;
                if (e.n > 1) break;
                if (fuses_bneck_tail(net, s, i)) { e.kind = LK_BNECK_TAIL; e.n = 2; }
                else if (fuses_bneck_seam(net, s, i)) { e.kind = LK_BNECK_SEAM; e.n = 2; }
                else if (fuses_bblockx3(net, s, i)) { e.kind = LK_BBLOCKX3; e.n = 2; }
                else if (fuses_bblock48(net, i)) { e.kind = LK_BBLOCK48; e.n = 2; }
                else if (tt_eligible(net, op, sb)) { e.kind = LK_TT; e.plan.cfg = tt_cfg(net, &op, 1, sb); }
                else {
                    e.kind = LK_CONV;
                    rc = choose_conv(net, op, sb, e.m[0]);
                    if (rc) return rc;
                }
                break;
            }
            case OP_UPADD: e.kind = LK_UPADD; break;
            case OP_HEAD: e.kind = LK_HEAD; break;
            case OP_SOFTMAX: e.kind = LK_TAIL; break;
            case OP_DECODE: e.kind = LK_DECODE; break;
        }
        for (int k = 0; k < e.n; ++k) {      // per covered op: the output forms this launch writes, the helper in front for its input twin
            e.m[k].out = out_forms(net, s, net.ops[i + k], e.kind);
            if (e.kind == LK_TT || e.kind == LK_BBLOCKX3) e.m[k].prep = prep_in(net, s, net.ops[i + k]);
        }
        if (e.kind == LK_BNECK_TAIL || e.kind == LK_BBLOCKX3 || e.kind == LK_BBLOCK48) e.m[0].out = Forms{false, false};      // stays in LDS
        i += e.n;
        s.launches.push_back(e);
    }
    s.dec = decode_at(net, s);
    for (Launch& e : s.launches) profile_launch(net, s, e);
    return SNCAL_OK;
}

}  // namespace

// the fused head's parameters that do not point into the workspace
void sncal::head_params(const sncal_hrnet& net, const Op& op, int sb, HeadParams& hp) {
    const Tensor& to = net.tensors[op.out];
    memset(&hp, 0, sizeof(hp));
    hp.range = net.d_range;
    hp.Cd = op.head_direct >= 0 ? net.tensors[op.head_direct].C : 0;
    hp.w0 = net.head_packed[HPK_W0].p; hp.bias0 = net.d_hb0; hp.w1 = net.head_packed[HPK_W1].p; hp.bias1 = net.d_hb1;
    hp.w0_32 = net.head_packed[HPK_W0_32].p; hp.w1_32 = net.head_packed[HPK_W1_32].p; hp.ks16 = net.head_ks16;
    hp.w0_32_lo = net.head_packed[HPK_W0_32_LO].p; hp.w1_32_lo = net.head_packed[HPK_W1_32_LO].p;
    hp.nsrc = op.head_nsrc;
    for (int s2 = 0; s2 < op.head_nsrc; ++s2) {
        const Tensor& ts = net.tensors[op.head_src[s2]];
        hp.Hs[s2] = ts.H; hp.Ws[s2] = ts.W;
        hp.sy[s2] = align_corners_ratio(ts.H, to.H);
        hp.sx[s2] = align_corners_ratio(ts.W, to.W);
    }
    hp.nfold = op.head_direct >= 0 ? op.head_nfold : 0;      // (a head without a direct tensor carries its folds in HeadX4Params)
    hp.ks1 = net.head_ks1;
    for (int s2 = 0; s2 < hp.nfold; ++s2) {
        const Tensor& tf = net.tensors[op.head_fold[s2]];
        hp.Cf[s2] = tf.C; hp.Hf[s2] = tf.H; hp.Wf[s2] = tf.W;
        hp.fsy[s2] = align_corners_ratio(tf.H, to.H);
        hp.fsx[s2] = align_corners_ratio(tf.W, to.W);
    }
    hp.N = sb; hp.H = to.H; hp.W = to.W; hp.HP = net.head_hp; hp.NQ = net.head_hp / 32; hp.LC = to.C;
}

void sncal::headx4_params(const sncal_hrnet& net, const Op& op, int sb, HeadX4Params& hp) {
    const Tensor& to = net.tensors[op.out];
    head_params(net, op, sb, hp.h);
    for (int f = 0; f < HEADX4_FOLD; ++f) {
        hp.fold[f] = nullptr; hp.Cf[f] = hp.Hf[f] = hp.Wf[f] = 0; hp.fsy[f] = hp.fsx[f] = 0.f;
        if (f >= op.head_nfold) continue;
        const Tensor& tf = net.tensors[op.head_fold[f]];
        hp.Cf[f] = tf.C; hp.Hf[f] = tf.H; hp.Wf[f] = tf.W;
        hp.fsy[f] = align_corners_ratio(tf.H, to.H);
        hp.fsx[f] = align_corners_ratio(tf.W, to.W);
    }
}

// the schedule of sub-batch size sb at the current layout, built on first use
int sncal::schedule_for(sncal_hrnet& net, int sb, Schedule** out) {
    for (Schedule& s : net.schedules)
        if (s.sb == sb) { *out = &s; return SNCAL_OK; }
    Schedule s;
    const int rc = build_schedule(net, sb, s);
    if (rc) return rc;
    net.schedules.push_back(std::move(s));
    *out = &net.schedules.back();
    return SNCAL_OK;
}
