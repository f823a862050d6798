// The activations of --act (networks/factory.py:195-200 of the reference) and their derivatives, shared by the normalise passes
// (norm.hip) and the attention gate (attgate.hip).
// HEAVY = false instantiations contain only relu / leakyrelu (the transcendental activations cost the streaming kernels
// ~10-20 % through code size and registers even when not selected)
#pragma once
#include "common.hpp"

template <bool HEAVY>
DEVI float act_fwd(float x, int act, float slope) {
  if (act == BRATS_ACT_RELU) return x > 0.f ? x : 0.f;
  if (act == BRATS_ACT_LEAKY) return x > 0.f ? x : x * slope;
  if constexpr (!HEAVY) return x;
  if (act == BRATS_ACT_ELU) return x > 0.f ? x : expm1f(x);
  if (act == BRATS_ACT_SWISH) return x / (1.f + __expf(-x));
  if (act == BRATS_ACT_MISH) {
    const float sp = x > 20.f ? x : log1pf(__expf(x));  // softplus with torch's threshold
    return x * tanhf(sp);
  }
  return x;
}
template <bool HEAVY>
DEVI float act_grad(float x, int act, float slope) {  // derivative at pre-activation x
  if (act == BRATS_ACT_RELU) return x > 0.f ? 1.f : 0.f;
  if (act == BRATS_ACT_LEAKY) return x > 0.f ? 1.f : slope;
  if constexpr (!HEAVY) return 1.f;
  if (act == BRATS_ACT_ELU) return x > 0.f ? 1.f : __expf(x);
  if (act == BRATS_ACT_SWISH) {
    const float sg = 1.f / (1.f + __expf(-x));
    return sg * (1.f + x * (1.f - sg));
  }
  if (act == BRATS_ACT_MISH) {
    const float sp = x > 20.f ? x : log1pf(__expf(x));
    const float th = tanhf(sp);
    const float sg = 1.f / (1.f + __expf(-x));
    return th + x * (1.f - th * th) * sg;
  }
  return 1.f;
}
