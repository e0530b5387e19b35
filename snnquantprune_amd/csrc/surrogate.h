// The surrogate derivatives of the spike functions, spiking_learning.py:139-241: what the BPTT
// scans of train_dense.hip and train_neuron.hip take as a template.
#pragma once

#include "common.h"

namespace snnqp {

template <int S>
__device__ __forceinline__ float surrogate_grad(float x) {
  if constexpr (S == SNNQP_SURR_FAST_SIGMOID) {        // :151-156, alpha = 10
    float d = 10.0f * fabsf(x) + 1.0f;
    return 1.0f / (d * d);
  } else if constexpr (S == SNNQP_SURR_ATAN) {         // :226-233, alpha = 2
    float p = 3.14159265358979323846f * x;
    return 1.0f / (1.0f + p * p);
  } else if constexpr (S == SNNQP_SURR_SLAYER) {       // :170-174
    return expf(-5.0f * fabsf(x));
  } else if constexpr (S == SNNQP_SURR_SMOOTH_STEP) {  // :188-192, [-0.5, 0.5)
    return (x < 0.5f && x >= -0.5f) ? 1.0f : 0.0f;
  } else {                                             // :206-211 piecewise_linear
    return fmaxf(1.0f - 2.0f * fabsf(x), 0.0f);
  }
}

}  // namespace snnqp
