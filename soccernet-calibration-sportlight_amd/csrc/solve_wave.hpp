// Part of the camera solve: included by solve.hip after its point-id masks and u64, and by labels.hip (one translation unit each).
// Wave reductions (shuffle and DPP forms), lane broadcasts, bit-set helpers, the RANSAC sampler and the best-hypothesis reduction.
#pragma once

namespace {

// ---- wave helpers ---------------------------------------------------------------------------------
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Reductions over aligned groups of W lanes (W = 8, 16, 32, 64) for the packed LM below: every lane ends with the sum / maximum of ITS
// group, and all groups of a wave hold the same points there, so every lane ends with the same bits.  Written with DPP moves -- quad
// swaps, row_half_mirror, row_mirror: three instructions per step and 64-bit value, no LDS round trip -- and, across the four rows of 16,
// v_readlane of the row leaders; as __shfl_xor in a non-inlined device function the same butterflies came out as ds_bpermute pairs
// (708 per iteration at W = 64 where the inlined round-4 code had 352 DPP moves: 2.6 -> 7.0 us per iteration on a 31-point fit, measured).
template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lane_value64(double v, int lane) {      // wave-uniform copy of lane `lane`'s value
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
template <int W, bool MAX>
__device__ __forceinline__ double wred_w(double v) {
    auto op = [](double a, double b) { return MAX ? fmax(a, b) : a + b; };
    v = op(v, dpp_mov64<0xB1>(v));                    // quad_perm [1,0,3,2]: lane ^ 1
    v = op(v, dpp_mov64<0x4E>(v));                    // quad_perm [2,3,0,1]: lane ^ 2
    v = op(v, dpp_mov64<0x141>(v));                   // row_half_mirror: the other quad of the 8
    if constexpr (W >= 16) v = op(v, dpp_mov64<0x140>(v));       // row_mirror: the other half of the row of 16
    if constexpr (W == 32) v = op(lane_value64(v, 0), lane_value64(v, 16));          // (both groups hold the same points: group 0's total)
    if constexpr (W == 64) v = op(op(lane_value64(v, 0), lane_value64(v, 16)), op(lane_value64(v, 32), lane_value64(v, 48)));
    return v;
}
template <int W> __device__ __forceinline__ double wsum_w(double v) { return wred_w<W, false>(v); }
template <int W> __device__ __forceinline__ double wmax_w(double v) { return wred_w<W, true>(v); }
__device__ __forceinline__ double bcast(double v, int lane) { return __shfl(v, lane, 64); }
__device__ __forceinline__ int popc64(u64 m) { return __popcll(m); }
__device__ __forceinline__ int kth_set_bit(u64 m, int k) {
    for (int i = 0; i < k; ++i) m &= m - 1;
    return __ffsll((long long)m) - 1;
}

// ---- RANSAC sampler (shared spec: oracle/solve.py::_mix / sample4) -------------------------------------
__device__ __forceinline__ u64 mix64(u64 h, u64 j) {
    u64 z = h * 0x9E3779B97F4A7C15ull + j * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ bool sample4(int h, int n, int (&idx)[4]) {
    int cnt = 0;
    for (int j = 0; j < 16 && cnt < 4; ++j) {
        const int c = (int)((mix64((u64)h, (u64)j) >> 32) % (u64)n);
        bool dup = false;
        for (int k = 0; k < cnt; ++k) dup |= idx[k] == c;
        if (!dup) idx[cnt++] = c;
    }
    return cnt == 4;
}

struct Best { int cnt; double s; int h; };
__device__ __forceinline__ bool better(const Best& a, const Best& b) {   // is a better than b
    return a.cnt > b.cnt || (a.cnt == b.cnt && (a.s < b.s || (a.s == b.s && a.h < b.h)));
}
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best q;
        q.cnt = __shfl_xor(v.cnt, o, 64); q.s = __shfl_xor(v.s, o, 64); q.h = __shfl_xor(v.h, o, 64);
        if (better(q, v)) v = q;
    }
    return v;
}

}  // namespace
