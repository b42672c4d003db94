// The op graph of an HRNet: conv layers in the reference's registration order, the flat op list over NHWC tensors with its launch
// groups, the three head formulations side by side, and the twin tensors of the fp8 / split engines.  Runs once, in sncal_hrnet_create.
//
// Mirrors the topology of HighResolutionNet (/root/reference/src/models/hrnet/hrnet.py:255-355 for the
// construction order / state-dict names, :437-511 for the forward) and of the line network
// (/root/reference/src/models/line/hrnet.py:30-249).  The network is lowered once into a flat list of
// ops over NHWC tensors:
//     INPUT   NCHW fp32 frames -> NHWC (channel-padded to one 16-byte k-group)
//     CONV    MFMA implicit-GEMM conv with folded BN, optional residual + ReLU   (conv.hpp)
//     UPADD   out = [relu](base + sum bilinear_up(src_i)); also used to write upsampled branches into a
//             channel slice of the head's concat tensor                             (ops.hip)
//     SOFTMAX NHWC fp32 logits -> NCHW fp32 (log-)softmax heatmaps
//     DECODE  D1 keypoint decode (decode.hip)
// Tensors get offsets inside one caller-provided workspace from a lifetime-based first-fit allocator, so a
// forward is a fixed sequence of kernel launches with no allocation.  Frames are processed in sub-batches
// (SNCAL_SUBBATCH, default 64) so that the activations of a sub-batch stay Infinity-Cache sized.
#include "hrnet_net.hpp"

using namespace sncal;

namespace {

struct Builder {
    sncal_hrnet& net;

    int add_layer(const std::string& name, const std::string& bn, int cin, int cout, int k, int stride, bool bias) {
        ConvLayer L;
        L.name = name; L.bn = bn; L.cin = cin; L.cout = cout; L.k = k; L.stride = stride; L.bias = bias;
        { const size_t q = name.find("stage"); if (q != std::string::npos && q + 5 < name.size()) L.stage = name[q + 5] - '0'; }
        net.layers.push_back(L);
        net.layer_by_name[name] = (int)net.layers.size() - 1;
        return (int)net.layers.size() - 1;
    }
    int new_tensor(int C, bool f32 = false) {
        Tensor t; t.C = C; t.f32 = f32;
        net.tensors.push_back(t);
        return (int)net.tensors.size() - 1;
    }
    int conv(const std::string& name, int in, bool relu, int res = -1, bool out_f32 = false) {
        auto it = net.layer_by_name.find(name);
        if (it == net.layer_by_name.end()) { set_error("internal: conv %s not enumerated", name.c_str()); return -1; }
        const ConvLayer& L = net.layers[it->second];
        Op op; op.type = OP_CONV; op.conv = it->second; op.in = in; op.res = res; op.relu = relu; op.out_f32 = out_f32;
        op.group = net.cur_group;
        const int cphys = out_f32 ? ((L.cout + 15) / 16) * 16 : L.cout;
        op.out = new_tensor(cphys, out_f32);
        net.ops.push_back(op);
        return op.out;
    }
    int upadd(int base, const std::vector<int>& srcs, bool relu, int C) {
        Op op; op.type = OP_UPADD; op.base = base; op.nsrc = (int)srcs.size(); op.relu = relu;
        for (size_t i = 0; i < srcs.size(); ++i) op.srcs[i] = srcs[i];
        op.group = net.cur_group;
        op.out = new_tensor(C);
        net.ops.push_back(op);
        return op.out;
    }
    void concat_part(int cat, int src, int coff, int dims_from, int dims_mul) {
        Op op; op.type = OP_UPADD; op.base = -1; op.nsrc = 1; op.srcs[0] = src; op.out = cat; op.out_coff = coff;
        op.dims_from = dims_from; op.dims_mul = dims_mul; op.group = net.cur_group;
        net.ops.push_back(op);
    }

    // ---- enumeration in the reference's registration order (hrnet.py:255-355) -------------------------
    void block_layers(const std::string& p, bool bottleneck, int inpl, int planes, bool ds) {
        if (!bottleneck) {
            add_layer(p + ".conv1", p + ".bn1", inpl, planes, 3, 1, false);
            add_layer(p + ".conv2", p + ".bn2", planes, planes, 3, 1, false);
            if (ds) add_layer(p + ".downsample.0", p + ".downsample.1", inpl, planes, 1, 1, false);
        } else {
            add_layer(p + ".conv1", p + ".bn1", inpl, planes, 1, 1, false);
            add_layer(p + ".conv2", p + ".bn2", planes, planes, 3, 1, false);
            add_layer(p + ".conv3", p + ".bn3", planes, planes * 4, 1, 1, false);
            if (ds) add_layer(p + ".downsample.0", p + ".downsample.1", inpl, planes * 4, 1, 1, false);
        }
    }

    void enumerate() {
        const sncal_hrnet_desc& d = net.desc;
        const std::string P = "model.";
        add_layer(P + "conv1", P + "bn1", 3, d.stem_width, 3, 2, false);
        add_layer(P + "conv2", P + "bn2", d.stem_width, d.stem_width, 3, 2, false);
        int inpl = 64;   // hard-coded in the reference (hrnet.py:273)
        for (int b = 0; b < d.stage1_blocks; ++b) {
            const bool ds = b == 0 && inpl != d.stage1_channels * 4;
            block_layers(fmt("%slayer1.%d", P.c_str(), b), true, inpl, d.stage1_channels, ds);
            inpl = d.stage1_channels * 4;
        }
        std::vector<int> pre{inpl};
        for (int si = 0; si < 3; ++si) {
            const int nb = d.num_branches[si];
            std::vector<int> cur(d.num_channels[si], d.num_channels[si] + nb);
            const std::string tn = fmt("%stransition%d", P.c_str(), si + 1);
            for (int i = 0; i < nb; ++i) {
                if (i < (int)pre.size()) {
                    if (cur[i] != pre[i])
                        add_layer(fmt("%s.%d.0", tn.c_str(), i), fmt("%s.%d.1", tn.c_str(), i), pre[i], cur[i], 3, 1, false);
                } else {
                    for (int j = 0; j < i + 1 - (int)pre.size(); ++j) {
                        const int cin = pre.back();
                        const int cout = (j == i - (int)pre.size()) ? cur[i] : cin;
                        add_layer(fmt("%s.%d.%d.0", tn.c_str(), i, j), fmt("%s.%d.%d.1", tn.c_str(), i, j), cin, cout, 3, 2, false);
                    }
                }
            }
            std::vector<int> inch = cur;
            for (int m = 0; m < d.num_modules[si]; ++m) {
                const std::string mn = fmt("%sstage%d.%d", P.c_str(), si + 2, m);
                for (int br = 0; br < nb; ++br)
                    for (int b = 0; b < d.num_blocks[si]; ++b) {
                        const int ch = d.num_channels[si][br];
                        block_layers(fmt("%s.branches.%d.%d", mn.c_str(), br, b), false, inch[br], ch, b == 0 && inch[br] != ch);
                        inch[br] = ch;
                    }
                for (int i = 0; i < nb; ++i)
                    for (int j = 0; j < nb; ++j) {
                        const std::string fn = fmt("%s.fuse_layers.%d.%d", mn.c_str(), i, j);
                        if (j > i) add_layer(fn + ".0", fn + ".1", inch[j], inch[i], 1, 1, false);
                        else if (j < i)
                            for (int k = 0; k < i - j; ++k) {
                                const int cout = (k == i - j - 1) ? inch[i] : inch[j];
                                add_layer(fmt("%s.%d.0", fn.c_str(), k), fmt("%s.%d.1", fn.c_str(), k), inch[j], cout, 3, 2, false);
                            }
                    }
            }
            pre = inch;
        }
        int last = 0;
        for (int c : pre) last += c;
        if (d.upscale > 1) last += d.stem_width;
        add_layer(P + "last_layer.0", P + "last_layer.1", last, last, 1, 1, true);
        add_layer(P + "last_layer.3", "", last, d.num_classes, 1, 1, true);
    }

    // ---- op graph (hrnet.py:437-511) -----------------------------------------------------------------
    int basic_block(const std::string& p, int x) {   // hrnet.py:42-58
        const int t = conv(p + ".conv1", x, true);
        int res = x;
        if (net.layer_by_name.count(p + ".downsample.0")) res = conv(p + ".downsample.0", x, false);
        return conv(p + ".conv2", t, true, res);
    }
    int bottleneck(const std::string& p, int x) {    // hrnet.py:79-99
        int t = conv(p + ".conv1", x, true);
        t = conv(p + ".conv2", t, true);
        int res = x;
        if (net.layer_by_name.count(p + ".downsample.0")) res = conv(p + ".downsample.0", x, false);
        return conv(p + ".conv3", t, true, res);
    }

    // The ops of one module's fuse section, re-ordered (the reference registers them output by output, hrnet.py:229-244): the stride-2
    // convolutions that START a fuse-down chain on the same input tensor become one launch group of consecutive ops, so that the executor
    // can run them as ONE launch that fetches the input once (conv.hpp conv_shared_s2_kernel).  A list scheduler over the section's own data
    // dependences: ops go out in the reference's order as they become ready; a group goes out as a whole, when its last member is ready
    // (members never depend on each other: a chain's first convolution reads a module input, and its accumulate operand comes from chains
    // of OTHER inputs).  Sums are accumulated in the reference's order: same bits.
    void schedule_fuse_section(size_t begin) {
        const size_t n = net.ops.size() - begin;
        if (n < 3) return;
        std::vector<Op> sec(net.ops.begin() + begin, net.ops.end());
        std::map<int, int> producer;                         // tensor -> op of the section that writes it
        for (size_t i = 0; i < n; ++i) if (sec[i].out >= 0) producer[sec[i].out] = (int)i;
        auto reads = [&](const Op& o) {
            std::vector<int> r{o.in, o.res, o.base, o.dims_from};
            for (int k = 0; k < o.nsrc; ++k) r.push_back(o.srcs[k]);
            return r;
        };
        std::vector<int> grp(n, -1);                          // group key per op: existing launch groups keep theirs
        std::map<int, std::vector<int>> shared;               // input tensor -> chain-starting stride-2 convolutions
        for (size_t i = 0; i < n; ++i) {
            const Op& o = sec[i];
            if (o.launch_group >= 0) { grp[i] = o.launch_group; continue; }
            if (o.type == OP_CONV && net.layers[o.conv].stride == 2 && net.layers[o.conv].k == 3 && !producer.count(o.in)) shared[o.in].push_back((int)i);
        }
        for (auto& kv : shared) {
            if (kv.second.size() < 2) continue;
            for (size_t k = 0; k < kv.second.size(); k += 3) {      // launches take up to three members
                if (kv.second.size() - k < 2) break;
                const int gid = net.n_launch_groups++;
                for (size_t q = k; q < std::min(kv.second.size(), k + 3); ++q) { grp[kv.second[q]] = gid; sec[kv.second[q]].launch_group = gid; sec[kv.second[q]].shared_in = true; }
            }
        }
        std::vector<char> done(n, 0);
        auto ready = [&](size_t i) {
            for (int t : reads(sec[i])) { auto it = t >= 0 ? producer.find(t) : producer.end(); if (it != producer.end() && it->second != (int)i && !done[it->second]) return false; }
            return true;
        };
        std::vector<Op> order;
        while (order.size() < n) {
            bool progressed = false;
            for (size_t i = 0; i < n && !progressed; ++i) {
                if (done[i] || !ready(i)) continue;
                std::vector<size_t> members{i};
                if (grp[i] >= 0) {
                    members.clear();
                    bool all = true;
                    for (size_t q = 0; q < n; ++q) if (grp[q] == grp[i]) { members.push_back(q); all = all && !done[q] && ready(q); }
                    if (!all) continue;
                }
                for (size_t q : members) { order.push_back(sec[q]); done[q] = 1; }
                progressed = true;
            }
            if (!progressed) {                               // (cannot happen with HRNet's fuse layers; keep the reference's order rather than loop)
                for (size_t i = 0; i < n; ++i) { sec[i].launch_group = net.ops[begin + i].launch_group; sec[i].shared_in = false; }
                return;
            }
        }
        std::copy(order.begin(), order.end(), net.ops.begin() + begin);
    }

    bool build() {
        const sncal_hrnet_desc& d = net.desc;
        const std::string P = "model.";
        enumerate();
        const int t_in = new_tensor(net.ge);
        { Op op; op.type = OP_INPUT; op.out = t_in; net.ops.push_back(op); }
        const int t_stem = conv(P + "conv1", t_in, true);
        int x = conv(P + "conv2", t_stem, true);
        for (int b = 0; b < d.stage1_blocks; ++b) x = bottleneck(fmt("%slayer1.%d", P.c_str(), b), x);
        std::vector<int> ys{x};
        const bool group_convs = env_flag(ENV_GROUP_CONVS);      // read per net: tests toggle it
        for (int si = 0; si < 3; ++si) {
            const int nb = d.num_branches[si];
            const std::string tn = fmt("%stransition%d", P.c_str(), si + 1);
            std::vector<int> xs;
            for (int i = 0; i < nb; ++i) {
                if (i < (int)ys.size()) {
                    if (net.layer_by_name.count(fmt("%s.%d.0", tn.c_str(), i))) xs.push_back(conv(fmt("%s.%d.0", tn.c_str(), i), ys[i], true));
                    else xs.push_back(ys[i]);
                } else {
                    int t = ys.back();
                    for (int j = 0; j < i + 1 - (int)ys.size(); ++j) t = conv(fmt("%s.%d.%d.0", tn.c_str(), i, j), t, true);
                    xs.push_back(t);
                }
            }
            for (int m = 0; m < d.num_modules[si]; ++m) {
                const std::string mn = fmt("%sstage%d.%d", P.c_str(), si + 2, m);
                // Branch 0 keeps block order (its conv pairs are pattern-matched into the fused BasicBlock kernel of the
                // bf16 path).  The other branches are emitted depth-major: the same-depth convs of branches 1..nb-1 are
                // independent and adjacent, so the executor can put them into ONE grouped launch (conv.hpp).
                bool plain = true;
                for (int br = 0; br < nb; ++br)
                    for (int b = 0; b < d.num_blocks[si]; ++b)
                        if (net.layer_by_name.count(fmt("%s.branches.%d.%d.downsample.0", mn.c_str(), br, b))) plain = false;
                if (group_convs && plain && nb > 2) {
                    for (int b = 0; b < d.num_blocks[si]; ++b) xs[0] = basic_block(fmt("%s.branches.0.%d", mn.c_str(), b), xs[0]);
                    for (int b = 0; b < d.num_blocks[si]; ++b) {
                        std::vector<int> t(nb);
                        const int g1 = net.n_launch_groups++;
                        for (int br = 1; br < nb; ++br) { t[br] = conv(fmt("%s.branches.%d.%d.conv1", mn.c_str(), br, b), xs[br], true); net.ops.back().launch_group = g1; }
                        const int g2 = net.n_launch_groups++;
                        for (int br = 1; br < nb; ++br) { xs[br] = conv(fmt("%s.branches.%d.%d.conv2", mn.c_str(), br, b), t[br], true, xs[br]); net.ops.back().launch_group = g2; }
                    }
                } else {
                    for (int br = 0; br < nb; ++br)
                        for (int b = 0; b < d.num_blocks[si]; ++b) xs[br] = basic_block(fmt("%s.branches.%d.%d", mn.c_str(), br, b), xs[br]);
                }
                std::vector<int> out(nb);
                const size_t fuse_begin = net.ops.size();
                for (int i = 0; i < nb; ++i) {                       // hrnet.py:229-244
                    int acc = xs[i];
                    const bool has_up = i < nb - 1;
                    for (int j = 0; j < i; ++j) {                    // fuse-down chains end with an accumulate
                        const std::string fn = fmt("%s.fuse_layers.%d.%d", mn.c_str(), i, j);
                        int t = xs[j];
                        for (int k = 0; k < i - j; ++k) {
                            const bool lastk = k == i - j - 1;
                            if (!lastk) t = conv(fmt("%s.%d.0", fn.c_str(), k), t, true);
                            else acc = conv(fmt("%s.%d.0", fn.c_str(), k), t, /*relu=*/!has_up && j == i - 1, acc);
                        }
                    }
                    if (has_up) {
                        std::vector<int> ups;
                        const bool grp = group_convs && nb - i - 1 >= 2;
                        const int gid = grp ? net.n_launch_groups++ : -1;      // the 1x1 convs of one fuse-up sum are independent
                        for (int j = i + 1; j < nb; ++j) {
                            ups.push_back(conv(fmt("%s.fuse_layers.%d.%d.0", mn.c_str(), i, j), xs[j], false));
                            net.ops.back().launch_group = gid;
                        }
                        acc = upadd(acc, ups, true, net.tensors[xs[i]].C);
                    }
                    out[i] = acc;
                }
                schedule_fuse_section(fuse_begin);
                xs = out;
            }
            ys = xs;
        }
        // head, reference formulation: upsample + concat + two 1x1 convs (hrnet.py:489-510; line/hrnet.py:236-248)
        net.n_public = (int)net.layers.size();
        net.t_stem = t_stem; net.t_branch0 = ys[0];
        net.l_head0 = net.layer_by_name[P + "last_layer.0"]; net.l_head1 = net.layer_by_name[P + "last_layer.3"];
        int catC = 0;
        for (int t : ys) catC += net.tensors[t].C;
        if (d.upscale > 1) catC += d.stem_width;
        net.cur_group = GRP_UNFUSED;
        const int cat = new_tensor(catC);
        int coff = 0;
        if (d.upscale > 1) { concat_part(cat, t_stem, coff, ys[0], d.upscale); coff += d.stem_width; }
        for (int t : ys) { concat_part(cat, t, coff, ys[0], d.upscale); coff += net.tensors[t].C; }
        const int hid = conv(P + "last_layer.0", cat, true);
        const int logits = conv(P + "last_layer.3", hid, false, -1, true);
        // head, fused formulation (head.hip): per-branch 1x1 products at native resolution + one fused kernel
        net.cur_group = GRP_FUSED;
        net.head_hp = ((catC + 31) / 32) * 32;
        net.head_m2 = (d.num_classes + 15) / 16;
        {
            Op hop; hop.type = OP_HEAD; hop.group = GRP_FUSED; hop.out = logits;
            int col = 0;
            std::vector<int> gathered;
            // upscale 4 (headx4.hip): the head is four times branch 0's size and no tensor sits there; the stem leads the folded sources
            if (d.upscale > 2) { hop.head_direct = -1; net.head_direct_coff = 0; net.head_direct_c = 0; gathered = ys; gathered.insert(gathered.begin(), t_stem); }
            else if (d.upscale > 1) { hop.head_direct = t_stem; net.head_direct_coff = 0; net.head_direct_c = d.stem_width; col = d.stem_width; gathered = ys; }
            else { hop.head_direct = ys[0]; net.head_direct_coff = 0; net.head_direct_c = net.tensors[ys[0]].C; col = net.head_direct_c; gathered.assign(ys.begin() + 1, ys.end()); }
            // narrow branches are upsampled inside the head kernel and appended to the stage-1 K dimension (their
            // columns of last_layer.0 follow the direct tensor's in concat order); the wide ones go through
            // t_i = W0_i . b_i at native resolution and are gathered
            net.head_k = net.head_direct_c;
            size_t first = 0;
            const int max_fold = hop.head_direct < 0 ? HEADX4_FOLD : HEAD_MAX_FOLD;
            while (first < gathered.size() && hop.head_nfold < max_fold && gathered.size() - first > 2 &&
                   net.head_k + net.tensors[gathered[first]].C <= 224 && net.tensors[gathered[first]].C % 8 == 0 && net.head_k % 8 == 0) {
                hop.head_fold[hop.head_nfold++] = gathered[first];
                net.head_k += net.tensors[gathered[first]].C;
                col += net.tensors[gathered[first]].C;
                ++first;
            }
            net.head_ks1 = net.head_k <= 64 ? 2 : net.head_k <= 160 ? 5 : 7;
            for (size_t gi = first; gi < gathered.size(); ++gi) {
                const int t = gathered[gi];
                const std::string nm = fmt("head.t%d", hop.head_nsrc);
                const int li = add_layer(nm, "", net.tensors[t].C, net.head_hp, 1, 1, false);
                net.layers[li].derived = true; net.layers[li].col_off = col;
                col += net.tensors[t].C;
                hop.head_src[hop.head_nsrc++] = conv(nm, t, false);
            }
            net.ops.push_back(hop);
        }
        // head, split formulation for the exact-fp32 engine: W0 . concat(up(b_i)) = sum_i up(W0_i . b_i) (a 1x1 convolution commutes
        // with bilinear interpolation): every source's 1x1 product at ITS OWN resolution (generic fp32 conv kernel; the direct
        // tensor's carries the folded-BN shift), one upsample_add with ReLU, then last_layer.3.  Same arithmetic type as the
        // reference formulation, different summation order (fp32 rounding level); 8.8 instead of 79.7 GMAC per frame at 960x540
        net.cur_group = GRP_SPLIT;
        {
            const int direct = d.upscale > 1 ? t_stem : ys[0];
            std::vector<int> rest;
            if (d.upscale > 1) rest = ys; else rest.assign(ys.begin() + 1, ys.end());
            if (d.upscale <= 2 && rest.size() <= 4) {      // (upscale 4: five interpolated sources and no base -- the reference formulation serves it)
                int col = 0;
                const ConvLayer& H0 = net.layers[net.l_head0];
                const int ld = add_layer("headx.d", "", net.tensors[direct].C, H0.cout, 1, 1, false);
                net.layers[ld].derived = true; net.layers[ld].col_off = col; net.layers[ld].derived_shift = true;
                col += net.tensors[direct].C;
                const int t_d = conv("headx.d", direct, false);
                std::vector<int> prods;
                for (size_t gi = 0; gi < rest.size(); ++gi) {
                    const std::string nm = fmt("headx.t%d", (int)gi);
                    const int li = add_layer(nm, "", net.tensors[rest[gi]].C, H0.cout, 1, 1, false);
                    net.layers[li].derived = true; net.layers[li].col_off = col;
                    col += net.tensors[rest[gi]].C;
                    prods.push_back(conv(nm, rest[gi], false));
                }
                const int hidden = upadd(t_d, prods, true, H0.cout);
                net.ops.back().group = GRP_SPLIT;
                Op op; op.type = OP_CONV; op.conv = net.l_head1; op.in = hidden; op.relu = false; op.out_f32 = true; op.group = GRP_SPLIT;
                op.out = logits;
                net.ops.push_back(op);
                net.has_split = true;
            }
        }
        net.cur_group = GRP_ALL;
        { Op op; op.type = OP_SOFTMAX; op.in = logits; op.out = new_tensor(d.num_classes, true);
          net.tensors[op.out].external_heat = true; net.t_heat = op.out; net.ops.push_back(op); }
        { Op op; op.type = OP_DECODE; op.in = net.t_heat; net.ops.push_back(op); }
        // split engines: the input tensor of every 3x3 stride-1 convolution of stages 2-4 gets a split twin (allocated only while a
        // two-team convolution reads it, see layout())
        if (net.x3)
            for (const Op& op : net.ops) {
                if (op.type != OP_CONV || op.group != GRP_ALL) continue;
                const ConvLayer& L = net.layers[op.conv];
                if (L.k == 3 && L.stride == 1 && L.stage >= 2 && L.cin % 16 == 0 && L.cout % 16 == 0 && net.tensors[op.in].C == L.cin && net.tensors[op.in].twin < 0) {
                    const int tw = new_tensor(L.cin);
                    net.tensors[tw].split = true;
                    net.tensors[op.in].twin = tw;
                }
            }
        // C5: every wide 3x3 stride-1 convolution may run in fp8 -> its input tensor gets an e4m3 twin (allocated only while
        // the layer is selected, see layout())
        if (net.fp8)
            for (const Op& op : net.ops) {
                if (op.type != OP_CONV) continue;
                const ConvLayer& L = net.layers[op.conv];
                if (L.k == 3 && L.stride == 1 && L.cin % 32 == 0 && L.cout % TT_COUT == 0 && net.tensors[op.in].C == L.cin && net.tensors[op.in].twin < 0) {
                    const int tw = new_tensor(L.cin);
                    net.tensors[tw].fp8 = true;
                    net.tensors[op.in].twin = tw;
                }
            }
        return true;
    }
};

}  // namespace

bool sncal::build_graph(sncal_hrnet& net) { return Builder{net}.build(); }
