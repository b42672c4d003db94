// Weights of an HRNet on their way to the device: balance (equalize_blocks) and range check of the split-fp16 engine, the (MI, G)
// choice of the generic kernel, and per layer one packing for every kernel that may read it.  The packed formats themselves belong to
// the kernels' headers (pack.hpp says where); this unit asks each format's predicate, calls its packer and uploads the bytes into the
// layer's / the head's DevBuf slots, which it owns.  Runs in sncal_hrnet_finalize.
#include "hrnet_net.hpp"

using namespace sncal;

namespace {

void release(DevBuf& b) { if (b.p) (void)hipFree(b.p); b = DevBuf{}; }
void release(float*& q) { if (q) (void)hipFree(q); q = nullptr; }

// host vector -> the device buffer in `slot`, in place of what the slot held
template <class T> int upload(DevBuf& slot, const std::vector<T>& host) {
    release(slot);
    SNCAL_CHECK_HIP(hipMalloc(&slot.p, host.size() * sizeof(T)));
    slot.bytes = host.size() * sizeof(T);
    SNCAL_CHECK_HIP(hipMemcpy(slot.p, host.data(), slot.bytes, hipMemcpyHostToDevice));
    return SNCAL_OK;
}
int upload(float*& slot, const std::vector<float>& host) {
    DevBuf b{slot, 0};
    const int rc = upload(b, host);
    slot = static_cast<float*>(b.p);
    return rc;
}

// choose (MI, G) for a layer: maximise useful/padded work x operand reuse among the instantiated variants
void choose_packing(sncal_hrnet& net, ConvLayer& L) {
    const int ge = net.ge;
    const int cout_frags = (L.cout + 15) / 16;
    double best = -1;
    for (int v = 0; v < net.nvariants; ++v) {
        const ConvVariant& V = net.variants[v];
        if (V.ks != L.k || V.stride != L.stride) continue;
        const ConvPackShape s{L.cin, L.cin_phys, L.cout, L.k, ge, V.mi, V.g};
        const int chunks = s.chunks(), nblk = s.nblk();
        const int nks = conv_nks(V.ks, V.g);
        const double k_eff = (double)(L.k * L.k * L.cin_phys / ge) / (double)(chunks * nks * 4);
        const double m_eff = (double)cout_frags / (nblk * V.mi);
        const double reuse = (double)(V.mi * 4) / (V.mi + 4);           // MFMAs per LDS fragment read (NI=4 nominal)
        const double per_chunk = (double)nks / (nks + 1.0);              // amortisation of the per-chunk sync/load
        // two workgroups per CU (<= 80 KB of LDS each) hide the staging rounds; judged on a nominal 2-wide tile
        const size_t stage2 = conv_stage_bytes(V.ks, V.stride, V.ni, V.mi, V.g, 2);
        // three resident workgroups (<= 53 KB, <= 168 VGPRs) measured 4 % faster on the latency-bound 48-channel class
        const double occ = stage2 > 80 * 1024 ? 0.55 : (stage2 <= 53 * 1024 && conv_wgs_per_cu(V.ks, V.ni, V.mi, V.g) == 3) ? 1.1 : 1.0;
        const double score = k_eff * m_eff * (0.55 + 0.45 * reuse / 2.4) * per_chunk * occ;
        if (score > best + 1e-9) { best = score; L.mi = V.mi; L.g = V.g; }
    }
    L.cout_frags = cout_frags;
    if (L.mi == 0) return;       // no variant (pack_weights reports it): no shape to ask
    const ConvPackShape s{L.cin, L.cin_phys, L.cout, L.k, ge, L.mi, L.g};
    L.nblk = s.nblk();
    L.chunks = s.chunks();
}

// every packing of a layer that a kernel of this engine may read (the predicates say which), in the slots of L.packed
int pack_layer(sncal_hrnet& net, ConvLayer& L) {
    const Folded W = L.folded();
    {
        std::vector<uint8_t> w;
        std::vector<float> bias;
        conv_pack_weights(W, L.shift.data(), ConvPackShape{L.cin, L.cin_phys, L.cout, L.k, net.ge, L.mi, L.g},
                          net.dtype == SNCAL_BF16 ? CONV_PACK_BF16 : net.x3 ? CONV_PACK_X3 : CONV_PACK_F32, w, bias);
        if (const int rc = upload(L.packed[PK_GENERIC], w)) return rc;
        if (const int rc = upload(L.d_bias, bias)) return rc;
    }
    if (net.dtype == SNCAL_BF16 && tt_shape_ok(L.k, L.stride, L.cin, L.cin_phys, L.cout)) {
        std::vector<uint16_t> w;
        tt_pack_weights(W, w);
        if (const int rc = upload(L.packed[PK_TT], w)) return rc;
        if (net.fp8) {
            std::vector<uint8_t> w8;
            tt8_pack_weights(W, w8, L.wscale);
            if (!L.d_oscale) SNCAL_CHECK_HIP(hipMalloc((void**)&L.d_oscale, (size_t)L.cout * 4));      // (filled by sncal_hrnet_calibrate_fp8)
            if (const int rc = upload(L.packed[PK_TT_FP8], w8)) return rc;
        }
    }
    if (net.x3 && net.dtype == SNCAL_F32) {
        std::vector<uint16_t> w;
        if (x3_shape_ok(L.k, L.stride, L.stage, L.cin, L.cin_phys, L.cout)) {
            L.x3_blk = ttx3_block(L.cout);
            ttx3_pack_weights(W, L.x3_blk, w);
            if (const int rc = upload(L.packed[PK_TT_X3], w)) return rc;
            if (L.cin == 48 && L.cout == 48) {
                bbx3_pack_weights(W, w);
                if (const int rc = upload(L.packed[PK_BBX3], w)) return rc;
            }
        }
        if (bnp_shape_ok(L.k, L.stride, L.cin, L.cout) && !L.derived) {
            bnp_pack_weights(W, w);
            if (const int rc = upload(L.packed[PK_BNP], w)) return rc;
        }
    }
    return SNCAL_OK;
}

// A fragments + biases of the fused head (head.hpp): head.hip's 16x16x32 packing (bf16 engine) and, when K1 is a multiple of 16, the
// 32x32x16 packing of head32.hip (bf16) and headx3.hip (split engines: hi and lo parts)
int pack_head(sncal_hrnet& net) {
    if (net.dtype != SNCAL_BF16 && !net.x3) return SNCAL_OK;
    const ConvLayer& H0 = net.layers[net.l_head0];
    const ConvLayer& H1 = net.layers[net.l_head1];
    if (!H1.is_set) { set_error("conv %s has no weights", H1.name.c_str()); return SNCAL_ERR_STATE; }
    // stage-1 K (head_k): the first concat columns (direct + folded branches)
    const HeadPackShape s{net.head_hp, net.head_m2, net.head_direct_c, net.head_direct_coff, net.head_k, net.head_ks1};
    if (!head_shape_ok(s)) return SNCAL_OK;      // fused kernel does not apply; the reference formulation is used
    const Folded W0 = H0.folded(), W1 = H1.folded();
    DevBuf* P = net.head_packed;
    net.head_ks16 = 0;
    if (s.K1 % 16 == 0) {
        std::vector<uint16_t> w0, w1, w0_lo, w1_lo;
        head32_pack_weights(W0, W1, s, net.x3, w0, w1, w0_lo, w1_lo);
        if (const int rc = upload(P[HPK_W0_32], w0)) return rc;
        if (const int rc = upload(P[HPK_W1_32], w1)) return rc;
        if (net.x3) {
            if (const int rc = upload(P[HPK_W0_32_LO], w0_lo)) return rc;
            if (const int rc = upload(P[HPK_W1_32_LO], w1_lo)) return rc;
        }
        net.head_ks16 = s.KS16();
    }
    if (!net.x3) {            // head.hip, bf16 only
        std::vector<uint16_t> w0, w1;
        head_pack_weights(W0, W1, s, w0, w1);
        if (const int rc = upload(P[HPK_W0], w0)) return rc;
        if (const int rc = upload(P[HPK_W1], w1)) return rc;
    }
    std::vector<float> b0, b1;
    head_pack_bias(H0.shift.data(), H0.cout, H1.shift.data(), H1.cout, s, b0, b1);
    if (const int rc = upload(net.d_hb0, b0)) return rc;
    return upload(net.d_hb1, b1);
}

// internal layers of the fused head are slices of last_layer.0 (BN scale folded, no shift)
int derive_head_slices(sncal_hrnet& net) {
    const ConvLayer& H0 = net.layers[net.l_head0];
    if (!H0.is_set) { set_error("conv %s has no weights", H0.name.c_str()); return SNCAL_ERR_STATE; }
    for (ConvLayer& L : net.layers) {
        if (!L.derived) continue;
        L.w.assign((size_t)L.cout * L.cin, 0.f);
        L.scale.assign(L.cout, 1.f); L.shift.assign(L.cout, 0.f);
        for (int co = 0; co < H0.cout; ++co) {
            L.scale[co] = H0.scale[co];
            if (L.derived_shift) L.shift[co] = H0.shift[co];
            for (int ci = 0; ci < L.cin; ++ci) L.w[(size_t)co * L.cin + ci] = H0.w[(size_t)co * H0.cin + L.col_off + ci];
        }
        L.is_set = true;
    }
    return SNCAL_OK;
}

// The split-fp16 engine (fp16x3) carries every operand as fp16 hi + fp16 lo: 22 significand bits for |v| in [2^-3, 65504], an ABSOLUTE
// resolution of 2^-25 below 2^-3 (lo is subnormal there), a hard clamp at +-65504 above (x3.hpp).  The reference's predict() is fp32 with
// no such limits (src/models/hrnet/metamodel.py:127-134), and a trained checkpoint may fold a near-dead BatchNorm channel
// (running_var ~ 0 -> scale gamma / sqrt(eps) = 316 gamma) into its weights.  So the engine refuses what it cannot represent instead of
// clamping it silently (x3_split_host saturates): any folded weight beyond 65504, or a layer whose weights sit so low that most of its
// weight mass has lost more than half of the 22 bits (|w| < 2^-14: hi itself is subnormal).  The caller falls back to dtype fp32
// (load_model does it by itself and says so).  Nothing switches the refusal off.
int x3_range_check(const sncal_hrnet& net) {
#if SNCAL_X3_F16
    if (!net.x3) return SNCAL_OK;
    for (const ConvLayer& L : net.layers) {
        if (!L.is_set || L.w.empty()) continue;
        const size_t per = L.w.size() / (size_t)L.cout;
        double mx = 0, mass = 0, low = 0;
        int mx_co = 0;
        bool outside = false;                                             // a folded weight beyond the range, infinite or NaN
        for (int co = 0; co < L.cout && !outside; ++co) {
            const double sc = L.scale.empty() ? 1.0 : (double)L.scale[co];
            for (size_t i = 0; i < per; ++i) {
                const double v = std::fabs((double)L.w[(size_t)co * per + i] * sc);
                if (!(v <= 65504.0)) { mx = v; mx_co = co; outside = true; break; }
                if (v > mx) { mx = v; mx_co = co; }
                mass += v;
                if (v < 6.103515625e-05) low += v;                        // 2^-14: fp16's smallest normal
            }
        }
        if (outside) {
            set_error("fp16x3 engine: folded weight %.6g of conv %s (output channel %d, BatchNorm scale %.6g) is outside the fp16 range "
                      "(65504): this checkpoint needs dtype='fp32'", mx, L.name.c_str(), mx_co, L.scale.empty() ? 1.0 : (double)L.scale[mx_co]);
            return SNCAL_ERR_RANGE;
        }
        if (mass > 0 && low > 0.5 * mass) {
            set_error("fp16x3 engine: %.0f %% of the folded weight mass of conv %s lies below 2^-14 (largest weight %.3g): fp16 halves keep fewer "
                      "than 11 of fp32's 24 bits there: this checkpoint needs dtype='fp32'", 100.0 * low / mass, L.name.c_str(), mx);
            return SNCAL_ERR_RANGE;
        }
    }
#endif
    return SNCAL_OK;
}

}  // namespace

// Power-of-two rebalancing of block-internal channels for the split-fp16 engine.  fp16 halves carry 22 significand bits only for |v| in
// [2^-3, 65504] and an ABSOLUTE 2^-25 below: a product w.x loses relative precision 2^-25 (1/|w| + 1/|x|), smallest when the weight and
// the activation it meets are of one size.  A trained checkpoint need not be balanced -- a BatchNorm with a small gamma in front of a
// convolution with large weights is the same function as the reverse (the reference computes in fp32 and cannot tell,
// src/models/hrnet/metamodel.py:127-134) -- and measured on a four-decade spread the engine drifted to |dlogp| 5e-3 with no flag
// (tests/test_range_guard_gpu.py).  Inside a block the balance is free to choose, EXACTLY: the output of conv1 + bn1 + ReLU of a BasicBlock
// (conv1 / conv2 of a Bottleneck) feeds one convolution only (src/models/hrnet/hrnet.py:42-58, 79-99), ReLU commutes with a positive factor,
// so row c of the producer (folded scale and shift) x 1/q_c and column c of the consumer x q_c, q_c a power of two, is the same network bit
// for bit in fp32.  m_c = size of the consumer column's large folded weights (90th percentile over its output channels of the largest tap:
// ONE outlier row -- a near-dead BatchNorm behind the consumer -- must not drag every column with it; that row is x3_range_check's to
// refuse), a_c = |shift_c| + |row c of the producer|_2 = size of the activation for unit-size inputs, l_c = round(log2(a_c / m_c) / 2) says
// how far apart the two are; an ordinary checkpoint (Kaiming-size weights, unit-size activations) sits at l = 2, the operating point every
// golden and parity workload of the build was measured at.  Channels with |l_c - 2| >= 4 are brought back to it (q_c = 2^(l_c - 2));
// everything else -- every channel of the build's own workloads -- is left untouched, bit for bit.  Tensors with several consumers
// (module outputs, residual streams) are not rebalanced: there the two range guards apply.  Host only (no HIP call).
// Rounds 5's host mirror did this in Python (HRNetHeatmap._equalize_blocks); it lives here so that every caller of the C ABI gets it.
int sncal::equalize_blocks(sncal_hrnet& net) {
    net.equalized = 0;
    net.equalize_done = true;
#if SNCAL_X3_F16
    if (!net.x3 || !net.equalize) return 0;
    const int MIN_LOG2 = 4, CENTRE = 2;
    auto split_name = [](const std::string& n, std::string& stem, std::string& leaf) {
        const size_t p = n.rfind('.');
        if (p == std::string::npos) { stem.clear(); leaf = n; } else { stem = n.substr(0, p); leaf = n.substr(p + 1); }
    };
    for (int i = 0; i + 1 < net.n_public; ++i) {
        ConvLayer& P = net.layers[i];
        ConvLayer& C = net.layers[i + 1];
        std::string stem, leaf, nstem, nleaf;
        split_name(P.name, stem, leaf);
        split_name(C.name, nstem, nleaf);
        const bool pair = (leaf == "conv1" && nleaf == "conv2") || (leaf == "conv2" && nleaf == "conv3");
        if (P.bn.empty() || stem != nstem || stem == "model" || !pair) continue;
        if (!P.is_set || !C.is_set || P.w.empty() || C.w.empty() || C.cin != P.cout) continue;
        const int nch = P.cout, taps2 = C.k * C.k;
        const size_t per1 = (size_t)P.cin * P.k * P.k;
        std::vector<double> col(C.cout);
        for (int c = 0; c < nch; ++c) {
            for (int co = 0; co < C.cout; ++co) {                 // consumer column c: largest tap of every output channel, folded
                double mx = 0;
                const float* w = &C.w[((size_t)co * C.cin + c) * taps2];
                for (int t = 0; t < taps2; ++t) mx = std::max(mx, std::fabs((double)w[t]));
                col[co] = mx * std::fabs((double)C.scale[co]);
            }
            std::sort(col.begin(), col.end());
            const double pos = 0.9 * (C.cout - 1);                // torch.quantile's linear interpolation
            const int lo = (int)std::floor(pos), hi = std::min(lo + 1, C.cout - 1);
            const double m = col[lo] + (col[hi] - col[lo]) * (pos - lo);
            double ss = 0;                                        // producer row c: size of its output
            const double sc = (double)P.scale[c];
            for (size_t j = 0; j < per1; ++j) { const double v = (double)P.w[(size_t)c * per1 + j] * sc; ss += v * v; }
            const double a = std::fabs((double)P.shift[c]) + std::sqrt(ss);
            if (!(m > 0) || !(a > 0) || !std::isfinite(m) || !std::isfinite(a)) continue;
            double lg = std::nearbyint(0.5 * std::log2(a / m)) - CENTRE;      // distance from the balance of an ordinary checkpoint
            if (std::fabs(lg) < MIN_LOG2) continue;
            lg = std::max(-60.0, std::min(60.0, lg));
            const float q = (float)std::exp2(lg), iq = (float)std::exp2(-lg);
            P.scale[c] *= iq;
            P.shift[c] *= iq;
            for (int co = 0; co < C.cout; ++co) {
                float* w = &C.w[((size_t)co * C.cin + c) * taps2];
                for (int t = 0; t < taps2; ++t) w[t] *= q;
            }
            ++net.equalized;
        }
    }
#endif
    return net.equalized;
}
int sncal::pack_weights(sncal_hrnet& net) {
    for (int i = 0; i < net.n_public; ++i)
        if (!net.layers[i].is_set) { set_error("conv %s has no weights", net.layers[i].name.c_str()); return SNCAL_ERR_STATE; }
    if (!net.equalize_done) equalize_blocks(net);   // fp16x3: before the head slices are derived and the range check reads the folded weights
    // physical Cin of every conv = channel count of its input tensor
    for (const Op& op : net.ops)
        if (op.type == OP_CONV) net.layers[op.conv].cin_phys = net.tensors[op.in].C;
    if (const int rc = derive_head_slices(net)) return rc;
    if (const int rc = pack_head(net)) return rc;
    if (const int rc = x3_range_check(net)) return rc;      // split-fp16 engine: the folded weights must live in fp16's range (SNCAL_ERR_RANGE)
    for (ConvLayer& L : net.layers) {
        if (!L.is_set) { set_error("conv %s has no weights", L.name.c_str()); return SNCAL_ERR_STATE; }
        choose_packing(net, L);
        if (L.mi == 0) { set_error("no kernel variant for conv %s (k=%d s=%d)", L.name.c_str(), L.k, L.stride); return SNCAL_ERR_STATE; }
        if (const int rc = pack_layer(net, L)) return rc;
        std::vector<float>().swap(L.w);
    }
    return SNCAL_OK;
}

void sncal::release_weights(sncal_hrnet& net) {
    for (ConvLayer& L : net.layers) {
        for (DevBuf& b : L.packed) release(b);
        release(L.d_bias); release(L.d_oscale);
    }
    for (DevBuf& b : net.head_packed) release(b);
    release(net.d_hb0); release(net.d_hb1);
}
