// What the two fused loss kernels (loss.hip, line_loss.hip) share besides their tiling: the load type of a lane that owns V
// consecutive columns, access to its elements, and the fp64 sum over a wave.
#pragma once
#include <hip/hip_runtime.h>

namespace sncal {

template <int V> struct Vec;
template <> struct Vec<4> { using type = float4; };
template <> struct Vec<1> { using type = float; };
__device__ __forceinline__ float lane_of(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ float lane_of(const float& v, int) { return v; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

}  // namespace sncal
