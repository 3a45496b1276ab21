// The int16 output rule of the resampler, shared by resample.hip and resample_stream.hip so that the two cannot drift apart:
// the float64 result x 32767, rounded to nearest (ties to even), saturated to [-32768, 32767]; a NaN has no int16 and gives 0.
#pragma once
#include <hip/hip_runtime.h>

namespace mn {

__device__ __forceinline__ short rs_to_i16(double y) {
  const double v = rint(y * 32767.0);                                 // to nearest, ties to even
  if (!(v == v)) return 0;                                            // a NaN has no int16: 0
  return (short)(int)(v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v));
}

}  // namespace mn
