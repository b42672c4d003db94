// The adaptive wing loss of one element, shared by the keypoint loss (loss.hip) and the line loss (line_loss.hip): both reference
// classes carry the same constants (hrnet/loss.py:76-79, line/loss.py:28-32) and the same formula (hrnet/loss.py:129-144,
// line/loss.py:78-108).
#pragma once
#include <hip/hip_runtime.h>

namespace sncal {

constexpr float AW_ALPHA = 2.1f, AW_OMEGA = 14.0f, AW_THETA = 0.5f;     // epsilon = 1

// `e` the prediction in [0, 1], `t` the target; fp32 step by step, theta / epsilon = 1/2 so the two pow() are exp2
__device__ __forceinline__ float adaptive_wing(float e, float t) {
    const float delta = fabsf(t - e), alpha_t = AW_ALPHA - t;
    const float P = exp2f(-alpha_t);                        // pow(theta / epsilon, alpha_t)
    const float P1 = exp2f(-(alpha_t - 1.0f));              // pow(theta / epsilon, alpha - target - 1)
    const float A = AW_OMEGA * (1.0f / (1.0f + P)) * alpha_t * P1;
    const float C = AW_THETA * A - AW_OMEGA * log1pf(P);
    return delta < AW_THETA ? AW_OMEGA * log1pf(powf(delta, alpha_t)) : A * delta - C;
}

}  // namespace sncal
