// input_quant.h -- the input quantisation rule (runner.cpp:158-164) shared by prep_input (misc_kernels.hip) and the
// image preprocessing kernel (preprocess.hip).  Device code; include after <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

namespace tf2 {

// runner.cpp:158-163: tmp = x * trans ; (int)(tmp > 0 ? tmp + 0.5 : tmp - 0.5) ; clamp, with tmp +- 0.5 evaluated in
// double and truncated toward zero.  Restated without double precision (the DP conversions run at a fraction of the
// VALU rate and this kernel is VALU bound): (double)tmp +- 0.5 is exact, so the result is sign * (floor|tmp| +
// (frac|tmp| >= 0.5)); floor and the fraction are exact in float.  |tmp| >= 2^31 or NaN: the reference's x86 cvttsd2si
// returns INT_MIN, which clamps to -128.
__device__ __forceinline__ int quant_input(float x, float trans) {
  const float tmp = x * trans;
  const float m = __builtin_fabsf(tmp);
  if (!(m < 2147483648.0f)) return -128;
  const float f = __builtin_floorf(m);
  float r = f + ((m - f) >= 0.5f ? 1.0f : 0.0f);
  r = tmp > 0 ? r : -r;
  r = r > 127.0f ? 127.0f : (r < -128.0f ? -128.0f : r);
  return (int)r;
}

}  // namespace tf2
