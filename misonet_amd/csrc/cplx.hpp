// What the float64 array kernels share (owpe.hip, oiva.hip, obf.hip; doa.hip, iva.hip, cacgmm.hip and jbf.hip where they spell the
// same expression): the finite tests, complex arithmetic on double2, the wave sum, the lane-group rule, and on the host the
// dispatch on the number of microphones and the copies of a debug call.  Kernel files only; one definition of each.  A kernel's
// bits depend on the form of these expressions -- the operand order, the parentheses, where a product may fuse -- so a change here
// changes every kernel that uses it, and all of them the same way.  A butterfly or a test that a kernel writes out in its own body
// stays written out: behind a call it compiled to other device code (oiva_k, the iva kernels and jbf_bin_k were tried).
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

namespace mn {

constexpr double F64_MAX = 1.7976931348623157e308;
constexpr float F32_MAX = 3.4028234663852886e38f;

// neither NaN nor infinite: one comparison with the largest finite value, false for a NaN
__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= F32_MAX; }
__device__ __forceinline__ bool finite(double v) { return fabs(v) <= F64_MAX; }

__host__ __device__ inline long long align16(long long n) { return (n + 15) & ~15LL; }

// ---- complex numbers as double2 -------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 c_wide(float2 v) { return make_double2((double)v.x, (double)v.y); }
__device__ __forceinline__ double2 c_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// acc + a b
__device__ __forceinline__ double2 c_fma(double2 acc, double2 a, double2 b) {
  return make_double2(acc.x + (a.x * b.x - a.y * b.y), acc.y + (a.x * b.y + a.y * b.x));
}
// acc - a b
__device__ __forceinline__ double2 c_fms(double2 acc, double2 a, double2 b) {
  return make_double2(acc.x - (a.x * b.x - a.y * b.y), acc.y - (a.x * b.y + a.y * b.x));
}
// acc - a conj(b)
__device__ __forceinline__ double2 c_fmsc(double2 acc, double2 a, double2 b) {
  return make_double2(acc.x - (a.x * b.x + a.y * b.y), acc.y - (a.y * b.x - a.x * b.y));
}
// 1 / p (Smith): no intermediate leaves the range of p
__device__ __forceinline__ double2 c_inv(double2 p) {
  if (fabs(p.x) >= fabs(p.y)) {
    const double r = p.y / p.x, d = p.x + p.y * r;
    return make_double2(1.0 / d, -r / d);
  }
  const double r = p.x / p.y, d = p.x * r + p.y;
  return make_double2(r / d, -1.0 / d);
}
// c ? a : b part by part: a conditional on the struct itself becomes a choice of addresses, and the struct scratch
__device__ __forceinline__ double2 c_sel(bool c, double2 a, double2 b) { return make_double2(c ? a.x : b.x, c ? a.y : b.y); }
// v of lane src of the group of G lanes
template <int G> __device__ __forceinline__ double2 c_from(double2 v, int src) {
  return make_double2(__shfl(v.x, src, G), __shfl(v.y, src, G));
}

// ---- lanes -----------------------------------------------------------------------------------------------------------------
// the sum of v over the 64 lanes of a wave by one butterfly, the same bits on every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}
// the lanes that own one M x M problem, lane j row j: the power of two that holds M
constexpr int lanes_for(int M) { return M <= 2 ? 2 : M <= 4 ? 4 : 8; }

// ---- the number of microphones as a template parameter ---------------------------------------------------------------------
// host: f(std::integral_constant<int, m>{}) for m = M in 2 .. 7, and m = 8 for every other M: the caller checks the range
template <class F> inline void with_m(int M, F&& f) {
  switch (M) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

// ---- host: the parts of a state block that a debug call copies out -----------------------------------------------------------
// bytes from state + off to dst, device to device on stream s, for every part whose dst is not null; the first error ends it
struct StatePart { void* dst; long long off, bytes; };
inline hipError_t copy_parts(const void* state, std::initializer_list<StatePart> parts, hipStream_t s) {
  for (const StatePart& p : parts) {
    if (!p.dst) continue;
    const hipError_t e = hipMemcpyAsync(p.dst, static_cast<const char*>(state) + p.off, p.bytes, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mn
