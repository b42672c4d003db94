// Shape inference + workspace layout for a sub-batch of `sb` frames of HxW: which head variant applies, which layers run on fp8 /
// split twins at this size, tensor lifetimes over the active ops, offsets from a first-fit allocator.  Cached per (sb, H, W).
#include "hrnet_net.hpp"

using namespace sncal;

// the layout and the launch schedules built on it are void: the next forward lays out again
void sncal::drop_layout(sncal_hrnet& net) {
    for (Schedule& s : net.schedules)
        for (Launch& e : s.launches) { if (e.plan.items) (void)hipFree(e.plan.items); if (e.plan.first) (void)hipFree(e.plan.first); }
    net.schedules.clear();
    net.lay_sb = -1;
}

namespace {

// which head formulation serves frames of HxW (net.use_fused / net.use_split; the same for every sub-batch size)
void choose_head(sncal_hrnet& net, int H, int W) {
    {   // does the fused head apply?  (bf16 path; the direct tensor must already sit at head resolution)
        auto half = [](int v) { return (v + 2 - 3) / 2 + 1; };
        const int sh = half(H), sw = half(W), bh = half(sh), bw = half(sw);
        const bool dims_ok = net.desc.upscale == 1 || (sh == bh * net.desc.upscale && sw == bw * net.desc.upscale);
        net.use_fused = net.fused_enabled && net.dtype == SNCAL_BF16 && dims_ok && net.head_packed[HPK_W0].p != nullptr;
        if (net.x3 && net.fused_enabled && dims_ok && net.desc.upscale == 2 && net.head_packed[HPK_W0_32_LO].p && net.head_ks16 == 13 && net.head_m2 == 4 &&
            headx3_enabled()) {
            // fp16x3: the fused split-arithmetic head (headx3.hip) when its gather boxes fit: branches 2 and 3 against the head's width
            // (the scales head_params will hand headx3_applies, before the tensors have their shapes).  headx3 gathers exactly TWO sources:
            // head_ks16 == 13 alone does not say so -- widths 144 / 160 / 320 / 400 fold only branch 0 (64 + 144 = 208 = 13 x 16) and
            // gather three -- so the head op's own source count decides with it; otherwise the split formulation below serves the head
            int nsrc = 0;
            for (const Op& op : net.ops) if (op.type == OP_HEAD) nsrc = op.head_nsrc;
            const int w2 = half(half(bw)), w3 = half(w2);
            net.use_fused = nsrc == 2 && head_boxes_fit(align_corners_ratio(w2, sw)) && head_boxes_fit(align_corners_ratio(w3, sw));
        }
        if (net.x3 && net.fused_enabled && net.desc.upscale == 4 && net.head_packed[HPK_W0_32_LO].p && net.head_ks16 == 13 && net.head_m2 == 4) {
            // fp16x3 at upscale 4: the fused head without a direct tensor (headx4.hip) when the stem and branches 0 and 1 are its three
            // blended sources, branches 2 and 3 its two gathered ones, and their boxes fit -- against a head of 4 x branch 0's size
            // (the scales headx4_params will hand headx4_applies); otherwise the reference formulation serves the head
            const Op* hop = nullptr;
            for (const Op& op : net.ops) if (op.type == OP_HEAD) hop = &op;
            if (hop && hop->head_direct < 0 && hop->head_nfold == HEADX4_FOLD && hop->head_nsrc == 2) {
                const int hh = bh * 4, hw = bw * 4, h1 = half(bh), w1 = half(bw), w2 = half(w1), w3 = half(w2);
                const int fh[HEADX4_FOLD] = {sh, bh, h1}, fw[HEADX4_FOLD] = {sw, bw, w1};
                int fc[HEADX4_FOLD];
                float fsy[HEADX4_FOLD], fsx[HEADX4_FOLD];
                for (int f = 0; f < HEADX4_FOLD; ++f) {
                    fc[f] = net.tensors[hop->head_fold[f]].C;
                    fsy[f] = align_corners_ratio(fh[f], hh); fsx[f] = align_corners_ratio(fw[f], hw);
                }
                const float gsx[2] = {align_corners_ratio(w2, hw), align_corners_ratio(w3, hw)};
                net.use_fused = headx4_fits(fc, fsy, fsx, gsx);
            }
        }
        net.use_split = !net.use_fused && net.has_split && net.dtype == SNCAL_F32 && dims_ok;
    }
}

// At upscale 4 the reference formulation holds a concat and a hidden tensor of the head's full width at FOUR times branch 0's size
// (784 channels x 540 x 960 for a 960x540 frame: 1.6 GB each in fp32), so the engines it serves run that many frames at a time that
// the two stay within this budget.  The fused head (headx4.hip) materialises neither and keeps the caller's sub-batch.
constexpr size_t X4_HEAD_BUDGET = (size_t)4 << 30;

}  // namespace

int sncal::sub_batch(sncal_hrnet& net, int B, int H, int W) {
    int sb = std::max(1, std::min(B, net.subbatch));
    if (net.desc.upscale != 4) return sb;
    choose_head(net, H, W);
    if (net.use_fused) return sb;
    auto half = [](int v) { return (v + 2 - 3) / 2 + 1; };
    const size_t px = (size_t)half(half(H)) * 4 * half(half(W)) * 4;
    const size_t per_frame = 2 * px * net.layers[net.l_head0].cout * net.esize;
    return (int)std::max<size_t>(1, std::min<size_t>(sb, X4_HEAD_BUDGET / per_frame));
}

int sncal::layout(sncal_hrnet& net, int sb, int H, int W) {
    if (net.lay_sb == sb && net.lay_h == H && net.lay_w == W) return SNCAL_OK;
    drop_layout(net);
    std::vector<Tensor>& T = net.tensors;
    choose_head(net, H, W);
    for (const Op& op : net.ops) {
        if (!op_active(net, op)) continue;
        switch (op.type) {
            case OP_INPUT: T[op.out].H = H; T[op.out].W = W; break;
            case OP_CONV: {
                const ConvLayer& L = net.layers[op.conv];
                const int pad = L.k / 2;
                T[op.out].H = (T[op.in].H + 2 * pad - L.k) / L.stride + 1;
                T[op.out].W = (T[op.in].W + 2 * pad - L.k) / L.stride + 1;
                break;
            }
            case OP_UPADD:
                if (op.base >= 0) { T[op.out].H = T[op.base].H; T[op.out].W = T[op.base].W; }
                else { T[op.out].H = T[op.dims_from].H * op.dims_mul; T[op.out].W = T[op.dims_from].W * op.dims_mul; }
                break;
            case OP_SOFTMAX: T[op.out].H = T[op.in].H; T[op.out].W = T[op.in].W; break;
            case OP_HEAD:
                if (op.head_direct >= 0) { T[op.out].H = T[op.head_direct].H; T[op.out].W = T[op.head_direct].W; }
                else { T[op.out].H = T[net.t_branch0].H * net.desc.upscale; T[op.out].W = T[net.t_branch0].W * net.desc.upscale; }
                break;
            case OP_DECODE: break;
        }
    }
    // C5: which layers run in fp8 = selected by sncal_hrnet_set_fp8_layers AND served by the two-team kernel at this size (the only
    // kernel that reads an e4m3 twin): twins, producers' outputs and the dispatch below all key on this ONE predicate, so a selected
    // layer that falls back to the generic kernel (SNCAL_CONV_TT=0, an odd channel offset, a size limit) simply stays bf16
    for (ConvLayer& L : net.layers) { L.fp8_on = false; L.x3_on = false; }
    for (const Op& op : net.ops) {
        if (op.type != OP_CONV || !op_active(net, op)) continue;
        ConvLayer& L = net.layers[op.conv];
        L.x3_on = net.x3 && L.packed[PK_TT_X3].p != nullptr && T[op.in].twin >= 0 && tt_eligible(net, op, sb);
        bool w_ok = net.fp8_widths.empty();
        for (int w : net.fp8_widths) w_ok = w_ok || w == L.cout;
        const bool s_ok = net.fp8_stages == 0 || ((net.fp8_stages >> L.stage) & 1u);
        L.fp8_on = net.fp8 && net.fp8_calibrated && !net.calibrating && L.packed[PK_TT_FP8].p != nullptr && w_ok && s_ok && L.stage >= 2 &&
                   T[op.in].twin >= 0 && tt_eligible(net, op, sb);
    }
    for (Tensor& t : T) { t.first = -1; t.last = -1; }
    for (size_t i = 0; i < net.ops.size(); ++i) {       // lifetimes over the active ops
        const Op& op = net.ops[i];
        if (!op_active(net, op)) continue;
        auto use = [&](int t) { if (t >= 0) T[t].last = std::max(T[t].last, (int)i); };
        use(op.in); use(op.res); use(op.base); use(op.dims_from); use(op.head_direct);
        for (int s2 = 0; s2 < op.nsrc; ++s2) use(op.srcs[s2]);
        for (int s2 = 0; s2 < op.head_nsrc; ++s2) use(op.head_src[s2]);
        for (int s2 = 0; s2 < op.head_nfold; ++s2) use(op.head_fold[s2]);
        if (op.out >= 0) { if (T[op.out].first < 0) T[op.out].first = (int)i; T[op.out].last = std::max(T[op.out].last, (int)i); }
    }
    for (Tensor& t : T) t.last_read = t.last;
    {   // Two consecutive convolutions of which the second reads the first one's output may run as ONE kernel (build_schedule: the fused
        // BasicBlocks, layer1's Bottleneck seams conv3 + next conv1, block 0's downsample tail).  That kernel reads the FIRST op's inputs
        // while it already writes the SECOND op's output, so for every such pair -- a superset of what the executor really fuses: the
        // predicates there depend on packing and sizes -- the first op's inputs outlive the second op and the second op's output exists
        // from the first op on.  (Until round 4 the second output was placed at step i + 1, after the first op's inputs had been
        // released: that they never overlapped was an accident of the first-fit geometry -- ADVICE r4.)
        int prev = -1;
        for (size_t i = 0; i < net.ops.size(); ++i) {
            const Op& op = net.ops[i];
            if (!op_active(net, op)) continue;
            if (prev >= 0 && op.type == OP_CONV && net.ops[prev].type == OP_CONV) {
                const Op& a = net.ops[prev];
                if (a.out >= 0 && (op.in == a.out || op.res == a.out)) {
                    auto keep = [&](int t) { if (t >= 0 && T[t].first >= 0) T[t].last = std::max(T[t].last, (int)i); };
                    keep(a.in); keep(a.res); keep(a.out);
                    if (op.out >= 0 && T[op.out].first > prev) T[op.out].first = prev;
                }
            }
            prev = (int)i;
        }
    }
    {   // the members of a launch group run concurrently: a tensor one of them reads must outlive ALL of them, and their
        // outputs must all exist from the first member on
        std::vector<int> gfirst(net.ops.size()), glast(net.ops.size());
        for (size_t i = 0; i < net.ops.size(); ++i) { gfirst[i] = glast[i] = (int)i; }
        for (size_t i = 0; i < net.ops.size();) {
            size_t j = i + 1;
            if (net.ops[i].launch_group >= 0)
                while (j < net.ops.size() && net.ops[j].launch_group == net.ops[i].launch_group) ++j;
            for (size_t k = i; k < j; ++k) { gfirst[k] = (int)i; glast[k] = (int)j - 1; }
            i = j;
        }
        for (Tensor& t : T) { if (t.first >= 0) t.first = gfirst[t.first]; if (t.last >= 0) t.last = glast[t.last]; }
    }
    {   // C5: an e4m3 twin lives exactly as long as its bf16 tensor, and only while an fp8 convolution reads it;
        // who writes each tensor, and whether anybody still reads the bf16 version (residuals, fuse layers, bf16 convs)
        net.producer.assign(T.size(), -1);
        net.need_bf16.assign(T.size(), 0);
        std::vector<char> twin_used(T.size(), 0);
        for (const Op& op : net.ops)
            if (op_active(net, op) && op.in >= 0 && op.type == OP_CONV && (net.layers[op.conv].fp8_on || net.layers[op.conv].x3_on) && T[op.in].twin >= 0)
                twin_used[op.in] = 1;
        for (size_t i = 0; i < net.ops.size(); ++i) {
            Op& op = net.ops[i];
            if (!op_active(net, op)) continue;
            if (op.out >= 0 && net.producer[op.out] < 0) net.producer[op.out] = (int)i;
            auto bf = [&](int t) { if (t >= 0) net.need_bf16[t] = 1; };
            // bf16x3: the second convolution of a BasicBlock takes its residual from the block input's split twin (the first convolution
            // read it), so that inside a chain of blocks nobody needs -- and no epilogue writes -- the fp32 form
            op.res_twin = op.type == OP_CONV && op.res >= 0 && net.layers[op.conv].x3_on && T[op.res].twin >= 0 && twin_used[op.res] &&
                          op.out_coff == 0 && T[op.out].C == net.layers[op.conv].cout && T[op.res].C == net.layers[op.conv].cout;
            if (!op.res_twin) bf(op.res);
            bf(op.base); bf(op.dims_from); bf(op.head_direct);
            for (int k = 0; k < op.nsrc; ++k) bf(op.srcs[k]);
            for (int k = 0; k < op.head_nsrc; ++k) bf(op.head_src[k]);
            for (int k = 0; k < op.head_nfold; ++k) bf(op.head_fold[k]);
            if (op.in >= 0) {
                const bool f8 = op.type == OP_CONV && (net.layers[op.conv].fp8_on || net.layers[op.conv].x3_on) && T[op.in].twin >= 0;
                if (f8) twin_used[op.in] = 1; else bf(op.in);
            }
        }
        for (size_t t = 0; t < T.size(); ++t)
            if (T[t].twin >= 0) {
                Tensor& w = T[T[t].twin];
                if (twin_used[t]) { w.first = T[t].first; w.last = T[t].last; } else { w.first = w.last = -1; }
            }
    }
    for (Tensor& t : T) if (t.twin >= 0) { T[t.twin].H = t.H; T[t.twin].W = t.W; }
    // first-fit allocator over op order
    struct Blk { size_t off, size; };
    std::vector<Blk> free_list;
    size_t top = 0;
    auto alloc = [&](size_t bytes) -> size_t {
        bytes = (bytes + 255) & ~(size_t)255;
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].size >= bytes) {
                const size_t off = free_list[i].off;
                free_list[i].off += bytes; free_list[i].size -= bytes;
                if (free_list[i].size == 0) free_list.erase(free_list.begin() + i);
                return off;
            }
        const size_t off = top; top += bytes; return off;
    };
    auto release = [&](size_t off, size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        free_list.push_back({off, bytes});
        std::sort(free_list.begin(), free_list.end(), [](const Blk& a, const Blk& b) { return a.off < b.off; });
        for (size_t i = 0; i + 1 < free_list.size();)
            if (free_list[i].off + free_list[i].size == free_list[i + 1].off) { free_list[i].size += free_list[i + 1].size; free_list.erase(free_list.begin() + i + 1); }
            else ++i;
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) { top = free_list.back().off; free_list.pop_back(); }
    };
    for (size_t i = 0; i < net.ops.size(); ++i) {
        for (size_t t = 0; t < T.size(); ++t)
            if (T[t].first == (int)i) {
                T[t].bytes = tensor_bytes(net, T[t], sb);
                T[t].offset = alloc(T[t].bytes);
            }
        for (size_t t = 0; t < T.size(); ++t)
            if (T[t].last == (int)i && T[t].first >= 0) release(T[t].offset, T[t].bytes);
    }
    // peak = max end offset
    size_t peak = 0;
    for (const Tensor& t : T) if (t.first >= 0) peak = std::max(peak, t.offset + ((t.bytes + 255) & ~(size_t)255));
    net.lay_bytes = peak;
    net.lay_sb = sb; net.lay_h = H; net.lay_w = W;
    return SNCAL_OK;
}
