// Weights of an HRNet on their way to the device: balance (equalize_blocks) and range check of the split-fp16 engine, the (MI, G)
// choice of the generic kernel, and one packing per kernel that reads the layer.  Runs in sncal_hrnet_finalize; the packed buffers
// are owned here (upload fills a slot, release_layer / release_head empty them all).
#include "hrnet_net.hpp"

using namespace sncal;

namespace {

void release(std::initializer_list<void**> slots) { for (void** q : slots) if (*q) { (void)hipFree(*q); *q = nullptr; } }

// host vector -> the device buffer in `slot`, in place of what the slot held
template <class P, class T> int upload(P*& slot, const std::vector<T>& host) {
    release({reinterpret_cast<void**>(&slot)});
    SNCAL_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&slot), host.size() * sizeof(T)));
    SNCAL_CHECK_HIP(hipMemcpy(slot, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    return SNCAL_OK;
}

// every packed buffer of a layer / of the head
void release_layer(ConvLayer& L) { release({&L.d_w, (void**)&L.d_bias, &L.d_w_tt, &L.d_w8, (void**)&L.d_oscale, &L.d_w_x3, &L.d_w_bbx, &L.d_w_bnp}); }
void release_head(sncal_hrnet& net) { release({&net.d_hw0, &net.d_hw1, &net.d_hw0_32, &net.d_hw1_32, &net.d_hw0_32l, &net.d_hw1_32l, (void**)&net.d_hb0, (void**)&net.d_hb1}); }

// choose (MI, G) for a layer: maximise useful/padded work x operand reuse among the instantiated variants
void choose_packing(sncal_hrnet& net, ConvLayer& L) {
    const int ge = net.ge;
    const int cout_frags = (L.cout + 15) / 16;
    double best = -1;
    for (int v = 0; v < net.nvariants; ++v) {
        const ConvVariant& V = net.variants[v];
        if (V.ks != L.k || V.stride != L.stride) continue;
        { static const int force_mi_s2 = env_int("SNCAL_FORCE_MI_S2", 0);     // tuning aids
          if (force_mi_s2 && L.k == 3 && L.stride == 2 && L.cin_phys >= 48 && V.mi != force_mi_s2 && cout_frags % force_mi_s2 == 0) continue; }
        { static const int force_g_s2 = env_int("SNCAL_FORCE_G_S2", 0);
          if (force_g_s2 && L.k == 3 && L.stride == 2 && L.cin_phys >= 48 && V.g != force_g_s2) continue; }
        const int chunks = (L.cin_phys + V.g * ge - 1) / (V.g * ge);
        const int nks = conv_nks(V.ks, V.g);
        const double k_eff = (double)(L.k * L.k * L.cin_phys / ge) / (double)(chunks * nks * 4);
        const int nblk = (cout_frags + V.mi - 1) / V.mi;
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
    L.nblk = (cout_frags + L.mi - 1) / L.mi;
    L.chunks = (L.cin_phys + L.g * ge - 1) / (L.g * ge);
}

inline uint16_t f2bf(float f) {   // round-to-nearest-even
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

int pack_layer(sncal_hrnet& net, ConvLayer& L) {
    const int ge = net.ge, KS = L.k, G = L.g, MI = L.mi;
    const int nks = conv_nks(KS, G);
    const size_t n16 = (size_t)L.nblk * L.chunks * nks * MI * 64;       // 16-byte vectors
    std::vector<uint8_t> host(n16 * 16, 0);
    for (int nb = 0; nb < L.nblk; ++nb)
        for (int c = 0; c < L.chunks; ++c)
            for (int s = 0; s < nks; ++s)
                for (int mi = 0; mi < MI; ++mi)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane & 15, g = lane >> 4;
                        const int kg = 4 * s + g;
                        const int tap = kg / G, cgi = kg % G;
                        const int co = (nb * MI + mi) * 16 + m;
                        uint8_t* dst = host.data() + ((((size_t)(nb * L.chunks + c) * nks + s) * MI + mi) * 64 + lane) * 16;
                        if (tap >= KS * KS || co >= L.cout) continue;
                        for (int e = 0; e < ge; ++e) {
                            const int ci = (c * G + cgi) * ge + e;
                            if (ci >= L.cin) continue;
                            const float v = L.w[(((size_t)co * L.cin + ci) * KS + tap / KS) * KS + tap % KS] * L.scale[co];
                            if (net.dtype == SNCAL_BF16) { const uint16_t b = f2bf(v); memcpy(dst + e * 2, &b, 2); }
                            else if (net.x3) {                  // [4 hi | 4 lo]: hi = rne16(w), lo = rne16(w - hi) (x3.hpp)
                                uint16_t h, l;
                                x3_split_host(v, &h, &l);
                                memcpy(dst + e * 2, &h, 2); memcpy(dst + 8 + e * 2, &l, 2);
                            }
                            else memcpy(dst + e * 4, &v, 4);
                        }
                    }
    std::vector<float> bias((size_t)L.nblk * MI * 16, 0.f);
    for (int co = 0; co < L.cout; ++co) bias[co] = L.shift[co];
    if (const int rc = upload(L.d_w, host)) return rc;
    return upload(L.d_bias, bias);
}

// Packing of a wide 3x3 stride-1 layer for the two-team kernel (conv_tt.hip): per (96-channel block nb, 32-channel chunk c)
// one 54 KB stage [tap 9][channel half 2][32-row block 3][lane 64] x 8 bf16, the A fragments of v_mfma_f32_32x32x16_bf16:
// lane l holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 32 + h * 16 + (l >> 5) * 8 + 0..7 of the tap.
bool tt_shape_ok(const sncal_hrnet& net, const ConvLayer& L) {
    return net.dtype == SNCAL_BF16 && L.k == 3 && L.stride == 1 && L.cin == L.cin_phys && L.cin % TT_CIN == 0 &&
           L.cout % TT_COUT == 0 && L.cout <= 480;
}

// bf16x3 engine: [nb][16-channel chunk c][tap 9][part: hi, lo][32-row block 3][lane 64] x 8 bf16 -- the two-team kernel's stage layout
// with the stage's two K = 16 steps holding the hi and the lo parts of the SAME 16 input channels: lane l holds output channel
// nb * 96 + mb * 32 + (l & 31) (zero rows above the layer's width: a 48-channel layer runs as one padded 96-channel block), input
// channels c * 16 + (l >> 5) * 8 + 0..7 of the tap; hi = bf16(w), lo = bf16(w - hi), w = folded weight in fp32.
bool x3_shape_ok(const sncal_hrnet& net, const ConvLayer& L) {
    return net.x3 && net.dtype == SNCAL_F32 && L.k == 3 && L.stride == 1 && L.stage >= 2 && L.cin == L.cin_phys && L.cin % 16 == 0 &&
           L.cout % 16 == 0 && L.cout <= 480;
}

int pack_layer_x3(sncal_hrnet& net, ConvLayer& L) {
    if (!x3_shape_ok(net, L)) return SNCAL_OK;
    L.x3_blk = L.cout % TT_COUT == 0 ? TT_COUT : 64;       // 48 channels: one padded 64-channel block (25 % zero rows) instead of 96 (50 %)
    const int MBk = L.x3_blk / 32;
    const int chunks = L.cin / 16, nblk = (L.cout + L.x3_blk - 1) / L.x3_blk;
    std::vector<uint16_t> host((size_t)nblk * chunks * 9 * 2 * MBk * 64 * 8, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int mb = 0; mb < MBk; ++mb)
                    for (int lane = 0; lane < 64; ++lane) {
                        // MFMA row r = lane & 31 computes channel x3_row_channel(r) of its block: quads 2 p, 2 p + 1 of a lane's accumulator
                        // registers are then 8 consecutive channels (conv_tt_body.inc x3_quad_channel, the twin-only epilogue)
                        const int r = lane & 31, rq = r >> 3, rh = (r >> 2) & 1, ri = r & 3;
                        const int co = nb * L.x3_blk + mb * 32 + 16 * (rq >> 1) + 8 * rh + 4 * (rq & 1) + ri;
                        if (co >= L.cout) continue;
                        uint16_t* hi = host.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + 0) * MBk + mb) * 64 + lane) * 8;
                        uint16_t* lo = host.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + 1) * MBk + mb) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) {
                            const int ci = c * 16 + (lane >> 5) * 8 + e;
                            const float w = L.w[(((size_t)co * L.cin + ci) * 3 + s / 3) * 3 + s % 3] * L.scale[co];
                            x3_split_host(w, &hi[e], &lo[e]);
                        }
                    }
    return upload(L.d_w_x3, host);
}

// bf16x3 engine: the fused 48-channel BasicBlock's own packing of a 48 -> 48 layer (bblockx3.hpp: 14 pair-steps of 6 KB)
int pack_layer_bbx3(sncal_hrnet& net, ConvLayer& L) {
    if (!x3_shape_ok(net, L) || L.cin != 48 || L.cout != 48) return SNCAL_OK;
    std::vector<uint16_t> host;
    bbx3_pack_weights(L.w.data(), L.scale.data(), [](float v, uint16_t* hi, uint16_t* lo) { x3_split_host(v, hi, lo); }, host);
    return upload(L.d_w_bbx, host);
}

// split engines: a 1x1 layer of layer1 in the fused Bottleneck seam's fragment order (bneckx3.hpp)
int pack_layer_bnp(sncal_hrnet& net, ConvLayer& L) {
    const bool shape = L.k == 1 && L.stride == 1 && ((L.cin == BNP_MID && L.cout == BNP_WIDE) || (L.cin == BNP_WIDE && L.cout == BNP_MID));
    if (!net.x3 || net.dtype != SNCAL_F32 || !shape || L.derived) return SNCAL_OK;
    std::vector<uint16_t> host;
    bnp_pack_weights(L.w.data(), L.scale.data(), L.cout, L.cin, [](float v, uint16_t* hi, uint16_t* lo) { x3_split_host(v, hi, lo); }, host);
    return upload(L.d_w_bnp, host);
}

int pack_layer_tt(sncal_hrnet& net, ConvLayer& L) {
    if (!tt_shape_ok(net, L)) return SNCAL_OK;
    const int chunks = L.cin / TT_CIN, nblk = L.cout / TT_COUT;
    std::vector<uint16_t> host((size_t)nblk * chunks * 9 * 2 * 3 * 64 * 8, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int h = 0; h < 2; ++h)
                    for (int mb = 0; mb < 3; ++mb)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint16_t* dst = host.data() + ((((((size_t)nb * chunks + c) * 9 + s) * 2 + h) * 3 + mb) * 64 + lane) * 8;
                            for (int e = 0; e < 8; ++e) {
                                const int ci = c * TT_CIN + h * 16 + (lane >> 5) * 8 + e;
                                dst[e] = f2bf(L.w[(((size_t)co * L.cin + ci) * 3 + s / 3) * 3 + s % 3] * L.scale[co]);
                            }
                        }
    return upload(L.d_w_tt, host);
}

// float -> OCP e4m3fn (1-4-3, bias 7, max 448, no infinities), round to nearest even, saturating
inline uint8_t f2fp8(float f) {
    if (!(f == f)) return 0x7f;
    const uint8_t sign = f < 0 ? 0x80 : 0;
    float a = std::fabs(f);
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0.0009765625f) return sign;                    // below half the smallest subnormal (2^-9 / 2): zero
    int e;
    float m = std::frexp(a, &e);                            // a = m * 2^e, m in [0.5, 1)
    int E = e - 1 + 7;                                      // biased exponent of 1.xxx * 2^(e-1)
    int q;
    if (E >= 1) {                                           // normal: 3 mantissa bits
        const float x = (m * 2.f - 1.f) * 8.f;
        q = (int)std::nearbyint(x);
        if (q == 8) { q = 0; ++E; }
        if (E > 15 || (E == 15 && q > 6)) return sign | 0x7e;
        return sign | (uint8_t)(E << 3) | (uint8_t)q;
    }
    q = (int)std::nearbyint(a * 512.f);                     // subnormal: multiples of 2^-9
    if (q >= 8) return sign | 0x08;
    return sign | (uint8_t)q;
}

// Packing of a wide 3x3 stride-1 layer for the fp8 variant of the two-team kernel: per (96-channel block nb, 64-channel chunk c)
// one 54 KB stage [tap 9][32-row block 3][half 2][lane 64] x 16 e4m3, the A operand of v_mfma_scale_f32_32x32x64_f8f6f4: lane l
// holds output channel nb * 96 + mb * 32 + (l & 31), input channels c * 64 + 32 (l >> 5) + 16 half + 0..15 of the tap (zeros
// beyond Cin).  One scale per output channel: wscale = max |w| / 448 over the folded weights of the channel.
int pack_layer_fp8(sncal_hrnet& net, ConvLayer& L) {
    if (!net.fp8 || !tt_shape_ok(net, L)) return SNCAL_OK;
    const int chunks = (L.cin + 63) / 64, nblk = L.cout / TT_COUT;
    L.wscale.assign(L.cout, 1.f);
    for (int co = 0; co < L.cout; ++co) {
        float mx = 0.f;
        for (size_t i = 0; i < (size_t)L.cin * 9; ++i) mx = std::max(mx, std::fabs(L.w[(size_t)co * L.cin * 9 + i] * L.scale[co]));
        L.wscale[co] = mx > 0.f ? mx / 448.f : 1.f;
    }
    std::vector<uint8_t> host((size_t)nblk * chunks * 9 * 3 * 2 * 64 * 16, 0);
    for (int nb = 0; nb < nblk; ++nb)
        for (int c = 0; c < chunks; ++c)
            for (int s = 0; s < 9; ++s)
                for (int mb = 0; mb < 3; ++mb)
                    for (int half = 0; half < 2; ++half)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int co = nb * TT_COUT + mb * 32 + (lane & 31);
                            uint8_t* dst = host.data() + (((((((size_t)nb * chunks + c) * 9 + s) * 3 + mb) * 2 + half) * 64) + lane) * 16;
                            for (int e = 0; e < 16; ++e) {
                                const int ci = c * 64 + 32 * (lane >> 5) + 16 * half + e;
                                if (ci < L.cin) dst[e] = f2fp8(L.w[(((size_t)co * L.cin + ci) * 3 + s / 3) * 3 + s % 3] * L.scale[co] / L.wscale[co]);
                            }
                        }
    if (!L.d_oscale) SNCAL_CHECK_HIP(hipMalloc((void**)&L.d_oscale, (size_t)L.cout * 4));      // (filled by sncal_hrnet_calibrate_fp8)
    return upload(L.d_w8, host);
}

// A fragments + biases of the fused head: head.hip's 16 x 16 x 32 layout (bf16 engine: d_hw0 / d_hw1) and, when K1 is a multiple of 16,
// the 32 x 32 x 16 layout of head32.hip (bf16: d_hw0_32 / d_hw1_32) and headx3.hip (split engines: every weight as hi + lo, the lo parts
// in d_hw0_32l / d_hw1_32l).  layout() picks the head variant from which of these are non-null and from head_ks16
int pack_head(sncal_hrnet& net) {
    if (net.dtype != SNCAL_BF16 && !net.x3) return SNCAL_OK;
    const ConvLayer& H0 = net.layers[net.l_head0];
    const ConvLayer& H1 = net.layers[net.l_head1];
    if (!H1.is_set) { set_error("conv %s has no weights", H1.name.c_str()); return SNCAL_ERR_STATE; }
    const int HP = net.head_hp, NQ = HP / 32, M2 = net.head_m2, Cd = net.head_direct_c, coff = net.head_direct_coff;
    const int K1 = net.head_k, KS1 = net.head_ks1;      // stage-1 K: the first K1 concat columns (direct + folded branches)
    if (Cd > 64 || M2 > 4 || K1 > KS1 * 32) return SNCAL_OK;      // fused kernel does not apply; the reference formulation is used
    net.head_ks16 = 0;
    if (K1 % 16 == 0) {       // A fragments of v_mfma_f32_32x32x16_bf16 -- lane l holds row h32_row_channel(l & 31) of the 32-row
        const int KS16 = K1 / 16, RB = (M2 * 16 + 31) / 32;                // block, k = 16 ks + 8 (l >> 5) + 0..7
        std::vector<uint16_t> v0((size_t)NQ * KS16 * 64 * 8, 0), v1((size_t)NQ * RB * 2 * 64 * 8, 0), v0l, v1l;
        if (net.x3) { v0l.assign(v0.size(), 0); v1l.assign(v1.size(), 0); }
        auto put = [&](std::vector<uint16_t>& hi, std::vector<uint16_t>& lo, size_t o, float w) {      // bf16: rounded; split engines: hi + lo
            if (net.x3) x3_split_host(w, &hi[o], &lo[o]); else hi[o] = f2bf(w);
        };
        for (int q = 0; q < NQ; ++q)
            for (int lane = 0; lane < 64; ++lane) {
                const int row = h32_row_channel(lane & 31), kb = (lane >> 5) * 8;
                const int ch = q * 32 + row;
                for (int ks = 0; ks < KS16 && ch < H0.cout; ++ks) {
                    const size_t o = (((size_t)q * KS16 + ks) * 64 + lane) * 8;
                    for (int e = 0; e < 8; ++e) put(v0, v0l, o + e, H0.w[(size_t)ch * H0.cin + coff + ks * 16 + kb + e] * H0.scale[ch]);
                }
                for (int rb = 0; rb < RB; ++rb)
                    for (int h = 0; h < 2; ++h) {
                        const int cls = rb * 32 + row;
                        if (cls >= H1.cout) continue;
                        const size_t o = ((((size_t)q * RB + rb) * 2 + h) * 64 + lane) * 8;
                        for (int e = 0; e < 8; ++e) {
                            const int k = q * 32 + h * 16 + kb + e;
                            if (k < H1.cin) put(v1, v1l, o + e, H1.w[(size_t)cls * H1.cin + k] * H1.scale[cls]);
                        }
                    }
            }
        if (const int rc = upload(net.d_hw0_32, v0)) return rc;
        if (const int rc = upload(net.d_hw1_32, v1)) return rc;
        if (net.x3) {
            if (const int rc = upload(net.d_hw0_32l, v0l)) return rc;
            if (const int rc = upload(net.d_hw1_32l, v1l)) return rc;
        }
        net.head_ks16 = KS16;
    }
    if (!net.x3) {            // head.hip, bf16 only
        std::vector<uint16_t> w0((size_t)NQ * 2 * KS1 * 64 * 8, 0), w1((size_t)NQ * M2 * 64 * 8, 0);
        for (int q = 0; q < NQ; ++q)
            for (int f = 0; f < 2; ++f)
                for (int ks = 0; ks < KS1; ++ks)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int m = lane & 15, gk = lane >> 4;
                        const int ch = q * 32 + (m >> 2) * 8 + f * 4 + (m & 3);      // row permutation, see head.hip
                        if (ch >= H0.cout) continue;
                        uint16_t* dst = w0.data() + ((((size_t)(q * 2 + f) * KS1 + ks) * 64) + lane) * 8;
                        for (int e = 0; e < 8; ++e) {
                            const int k = ks * 32 + gk * 8 + e;
                            if (k < K1) dst[e] = f2bf(H0.w[(size_t)ch * H0.cin + coff + k] * H0.scale[ch]);
                        }
                    }
        for (int q = 0; q < NQ; ++q)
            for (int mi = 0; mi < M2; ++mi)
                for (int lane = 0; lane < 64; ++lane) {
                    const int cls = mi * 16 + (lane & 15), gk = lane >> 4;
                    if (cls >= H1.cout) continue;
                    uint16_t* dst = w1.data() + (((size_t)(q * M2 + mi) * 64) + lane) * 8;
                    for (int e = 0; e < 8; ++e) {
                        const int k = q * 32 + gk * 8 + e;
                        if (k < H1.cin) dst[e] = f2bf(H1.w[(size_t)cls * H1.cin + k] * H1.scale[cls]);
                    }
                }
        if (const int rc = upload(net.d_hw0, w0)) return rc;
        if (const int rc = upload(net.d_hw1, w1)) return rc;
    }
    std::vector<float> b0(HP, 0.f), b1((size_t)std::max(M2 * 16, 64), 0.f);      // head32's decode epilogue reads 64 bias slots whatever C
    for (int co = 0; co < H0.cout; ++co) b0[co] = H0.shift[co];
    for (int c = 0; c < H1.cout; ++c) b1[c] = H1.shift[c];
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
// (load_model does it by itself and says so).  SNCAL_X3_RANGE_CHECK=0 switches the refusal off (tests of the run-time range flag).
int x3_range_check(const sncal_hrnet& net) {
#if SNCAL_X3_F16
    if (!net.x3) return SNCAL_OK;
    static const bool off = getenv("SNCAL_X3_RANGE_CHECK") && atoi(getenv("SNCAL_X3_RANGE_CHECK")) == 0;
    if (off) return SNCAL_OK;
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
        for (auto pack : {pack_layer, pack_layer_tt, pack_layer_fp8, pack_layer_x3, pack_layer_bbx3, pack_layer_bnp})      // each packs what its kernel serves
            if (const int rc = pack(net, L)) return rc;
        std::vector<float>().swap(L.w);
    }
    return SNCAL_OK;
}

void sncal::release_weights(sncal_hrnet& net) {
    for (ConvLayer& L : net.layers) release_layer(L);
    release_head(net);
}
