// The signals the waveform scorers read (score.hip, bss.hip, stoi.hip, reverb.hip, srmr.hip), and what those files share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mn {

// A strided view of a batch of signals: element (item b, source c, sample m) at p[b sb + c ss + m st], strides in elements;
// float32, or int16 where i16 is set.  The mixture is a view of one source per item (ss = 0); a view that is not there has
// p = nullptr and is never picked.  An int16 sample q stands for q / 32767.  Where that factor is applied differs, and the
// results are held bit for bit, so the two ways are two loads:
//   sig_raw   the number as stored; the kernel sums those and scales once after the sum by sig_unit (score.hip, bss.hip and
//             the resampler of stoi.hip, whose two loops use SIG_I16_UNIT directly)
//   sig_load  the value, divided at the load (reverb.hip, srmr.hip)
struct SigView { const void* p; long long sb, ss, st; int i16; };

constexpr double SIG_I16_UNIT = 1.0 / 32767.0;
inline double sig_unit(const SigView& v) { return v.i16 ? SIG_I16_UNIT : 1.0; }

// the samples of item b that count: n_valid[b] held to [0, n], or n where there is no n_valid
__device__ __forceinline__ long long sig_nv(const int* n_valid, int b, long long n) {
  if (!n_valid) return n;
  const long long v = n_valid[b];
  return v < 0 ? 0 : (v < n ? v : n);
}

// signal s of item b among R references, E estimates and the mixture, in that order: its view, and in *base the offset of
// its sample 0.  R = 0 picks between the estimates and the mixture.
__device__ __forceinline__ const SigView& sig_pick(const SigView& ref, const SigView& est, const SigView& mix, int R, int E,
                                                   int s, int b, long long* base) {
  const SigView& v = s < R ? ref : (s < R + E ? est : mix);
  const int src = s < R ? s : (s < R + E ? s - R : 0);
  *base = (long long)b * v.sb + (long long)src * v.ss;
  return v;
}

__device__ __forceinline__ float sig_raw(const SigView& v, long long base, long long m) {
  return v.i16 ? (float)reinterpret_cast<const int16_t*>(v.p)[base + m * v.st]
               : reinterpret_cast<const float*>(v.p)[base + m * v.st];
}
__device__ __forceinline__ double sig_load(const SigView& v, long long base, long long m) {
  return v.i16 ? (double)reinterpret_cast<const int16_t*>(v.p)[base + m * v.st] / 32767.0
               : (double)reinterpret_cast<const float*>(v.p)[base + m * v.st];
}

// the 256 values v of a workgroup added by a fixed tree; every thread gets the sum.  s[256] is free again on return.
template <typename T>
__device__ __forceinline__ T sig_tree(T* s, T v, int t) {
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (t < k) s[t] += s[t + k];
    __syncthreads();
  }
  return s[0];
}

// host: the modified Bessel function I0 of the Kaiser windows as its power series sum_k ((x / 2)^k / k!)^2: every term
// positive, converged long before 64 terms for the beta in use
inline double sig_i0(double x) {
  double s = 1.0, t = 1.0;
  for (int k = 1; k < 64; ++k) {
    t *= (x / 2.0) / k;
    s += t * t;
  }
  return s;
}

}  // namespace mn
