// The two pieces of the reference's target heatmap that target.hip (writes the target) and loss.hip (rebuilds it in registers)
// must evaluate identically: the 1D Gaussian of loss.py:7-18 and the visibility test of loss.py:49.
#pragma once
#include <hip/hip_runtime.h>

namespace sncal {

// -(torch.div(x - mu, sigma) ** 2) / 2.0, fp32 step by step as torch evaluates it: the argument of the exp below, and the exact
// logarithm of the Gaussian before its rounding to fp32
__device__ __forceinline__ float gauss1_arg(float x, float mu, float sigma) {
    const float d = (x - mu) / sigma;
    return -(d * d) / 2.0f;
}

// exp is float32(exp(float64)), i.e. correctly rounded (torch's CPU exp is within 1 ulp of that: tests/test_target_gpu.py)
__device__ __forceinline__ float gauss1(float x, float mu, float sigma) { return (float)exp((double)gauss1_arg(x, mu, sigma)); }

// torch.any(keypoints == 1, dim=-1) over ALL three components: a point whose x or y is exactly 1.0 counts as visible even with
// flag 0 (mirrored, not fixed)
__device__ __forceinline__ int kp_visible(float x, float y, float flag) { return (x == 1.0f) | (y == 1.0f) | (flag == 1.0f); }

}  // namespace sncal
