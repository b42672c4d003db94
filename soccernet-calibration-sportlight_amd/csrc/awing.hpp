// The adaptive wing loss of one element and its derivative, shared by the keypoint loss (loss.hip) and the line loss (line_loss.hip): both reference
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

// d adaptive_wing / d delta, as torch autograd differentiates the formula above with the target held fixed:
//   delta < theta:  omega * a * delta^(a-1) / (1 + delta^a),  delta^a formed as delta^(a-1) * delta (one pow)
//   otherwise:      A(t), the slope of the linear branch (the two are equal at delta = theta)
// The caller multiplies by sign(e - t) and takes 0 at delta == 0 (sign(0) = 0; delta^(a-1) is infinite there when t > 1.1).
__device__ __forceinline__ float adaptive_wing_slope(float delta, float t) {
    const float alpha_t = AW_ALPHA - t;
    if (delta < AW_THETA) {
        const float pw = powf(delta, alpha_t - 1.0f);
        return AW_OMEGA * alpha_t * pw / (1.0f + pw * delta);
    }
    const float P = exp2f(-alpha_t);
    const float P1 = exp2f(-(alpha_t - 1.0f));
    return AW_OMEGA * (1.0f / (1.0f + P)) * alpha_t * P1;
}

// the wing term of a loss gradient with respect to the prediction `e`: slope * sign(e - t)
__device__ __forceinline__ float adaptive_wing_grad(float e, float t) {
    const float delta = fabsf(t - e);
    if (delta == 0.f) return 0.f;
    const float s = adaptive_wing_slope(delta, t);
    return e > t ? s : -s;
}

}  // namespace sncal
