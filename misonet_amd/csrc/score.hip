// Scoring of separated output against clean references on the device (C ABI misonet_score_wave / misonet_score_spec in
// net.hip; the definitions are restated in NumPy in tests/score_ref.py).
//
//   score_wave_k       part[item][segment][.] = the sums  S e_i, S e_i^2, S r_j, S r_j^2, S e_i r_j  of one 4096-sample segment
//   score_wave_fold_k  stats[item][i][j] = (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j): the segments added in segment order
//   score_spec_k       part[item][f][i][j] = sum_t |Re e - Re r| + |Im e - Im r| + | sqrt(Re e^2 + Im e^2 + 1e-8) - |r| |
//   score_spec_fold_k  pair[item][i][j] = the bins added in bin order; the cheapest permutation (uPIT) and its value
//
// Every reduction runs in a fixed order and nothing is accumulated with atomics: the result of an item is bit-reproducible
// and does not depend on the batch it sits in or on its position there (as pit_dist_k / pit_pick_k, mvdr.hip).
#include "kernels.hpp"

namespace mn {

constexpr int SCORE_SEG = 4096;       // samples per workgroup of score_wave_k: 2 rounds x 256 lanes x 8 samples
constexpr int SCORE_GRP = 8;          // consecutive samples per lane and round: 16 bytes of int16, 2 x 16 bytes of float32

__device__ __forceinline__ void load8(const int16_t* p, float* v) {
  union { uint4 u; int16_t s[8]; } x;
  x.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = (float)x.s[k];
}
__device__ __forceinline__ void load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// 8 samples [m0, m0 + 8) of one signal: one 16-byte run where the view is sample-contiguous and the run lies inside the
// array, otherwise one bounds-checked load per sample.  Samples at or past nv (<= n) read as 0.
template <typename T>
__device__ __forceinline__ void load_group(const T* base, long long st, bool vec, long long m0, long long n, long long nv,
                                           float* v) {
  if (vec && m0 + SCORE_GRP <= n) {
    load8(base + m0, v);
  } else {
#pragma unroll
    for (int k = 0; k < SCORE_GRP; ++k) v[k] = m0 + k < n ? (float)base[(m0 + k) * st] : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < SCORE_GRP; ++k) v[k] = m0 + k < nv ? v[k] : 0.0f;
}

struct WaveView { SigView v; int vec; };                               // vec: the view takes 16-byte loads (wave_vec)

// grid (segments, items), 256 threads.  A lane adds its 16 samples of every signal in sample order, in double (the product
// of two float32 values is exact there); 64-lane butterfly, then the four waves in wave order.
// part [item][segment][2E + 2R + E R]: S e (E), S e^2 (E), S r (R), S r^2 (R), S e_i r_j (E R)
template <int E, int R, typename EstT>
__global__ __launch_bounds__(256) void score_wave_k(const WaveView ve, const WaveView vr, long long n, const int* n_valid,
                                                    double* part) {
  constexpr int NS = 2 * E + 2 * R + E * R;
  __shared__ double s_tmp[4][NS];
  const int seg = blockIdx.x, b = blockIdx.y;
  const long long nv = sig_nv(n_valid, b, n);
  const EstT* pe = reinterpret_cast<const EstT*>(ve.v.p) + (long long)b * ve.v.sb;
  const float* pr = reinterpret_cast<const float*>(vr.v.p) + (long long)b * vr.v.sb;
  double acc[NS];
#pragma unroll
  for (int i = 0; i < NS; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int round = 0; round < SCORE_SEG / (256 * SCORE_GRP); ++round) {
    const long long m0 = (long long)seg * SCORE_SEG + (long long)round * (256 * SCORE_GRP) + (long long)threadIdx.x * SCORE_GRP;
    if (m0 >= nv) continue;                                            // nothing but zeros: the sums do not move
    float e[E][SCORE_GRP], r[R][SCORE_GRP];
#pragma unroll
    for (int i = 0; i < E; ++i) load_group(pe + (long long)i * ve.v.ss, ve.v.st, ve.vec != 0, m0, n, nv, e[i]);
#pragma unroll
    for (int j = 0; j < R; ++j) load_group(pr + (long long)j * vr.v.ss, vr.v.st, vr.vec != 0, m0, n, nv, r[j]);
#pragma unroll
    for (int k = 0; k < SCORE_GRP; ++k) {
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const double x = (double)e[i][k];
        acc[i] += x;
        acc[E + i] += x * x;
#pragma unroll
        for (int j = 0; j < R; ++j) acc[2 * E + 2 * R + i * R + j] += x * (double)r[j][k];
      }
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const double y = (double)r[j][k];
        acc[2 * E + j] += y;
        acc[2 * E + R + j] += y * y;
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    double v = acc[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) s_tmp[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    const int i = threadIdx.x;
    part[((long long)b * gridDim.x + seg) * NS + i] = (s_tmp[0][i] + s_tmp[1][i]) + (s_tmp[2][i] + s_tmp[3][i]);
  }
}

// grid (items), 128 threads.  ce = the value one unit of the estimate stands for (1 / 32767 for int16, 1 for float32),
// applied once to the folded sums.  stats [item][E][R][5]
__global__ __launch_bounds__(128) void score_wave_fold_k(const double* part, int nseg, int E, int R, double ce, double* stats) {
  __shared__ double s_sum[2 * 5 + 2 * 4 + 5 * 4];
  const int NS = 2 * E + 2 * R + E * R;
  const int b = blockIdx.x;
  if ((int)threadIdx.x < NS) {
    const double* q = part + (long long)b * nseg * NS + threadIdx.x;
    double a = 0.0;
    for (int s = 0; s < nseg; ++s) a += q[(long long)s * NS];          // fixed order: segment 0, 1, ...
    s_sum[threadIdx.x] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < E * R * 5) {
    const int c = threadIdx.x % 5, ij = threadIdx.x / 5, i = ij / R, j = ij % R;
    double v;
    switch (c) {
      case 0: v = s_sum[i] * ce; break;
      case 1: v = s_sum[2 * E + j]; break;
      case 2: v = s_sum[E + i] * (ce * ce); break;
      case 3: v = s_sum[2 * E + R + j]; break;
      default: v = s_sum[2 * E + 2 * R + ij] * ce; break;
    }
    stats[(long long)b * E * R * 5 + threadIdx.x] = v;
  }
}

template <int E, int R, typename EstT>
static void wave_launch(const WaveView& ve, const WaveView& vr, int B, long long n, int nseg, const int* n_valid, double* part,
                        hipStream_t s) {
  hipLaunchKernelGGL((score_wave_k<E, R, EstT>), dim3(nseg, B), dim3(256), 0, s, ve, vr, n, n_valid, part);
}
template <int E, typename EstT>
static hipError_t wave_r(const WaveView& ve, const WaveView& vr, int B, int R, long long n, int nseg, const int* n_valid,
                         double* part, hipStream_t s) {
  switch (R) {
    case 1: wave_launch<E, 1, EstT>(ve, vr, B, n, nseg, n_valid, part, s); break;
    case 2: wave_launch<E, 2, EstT>(ve, vr, B, n, nseg, n_valid, part, s); break;
    case 3: wave_launch<E, 3, EstT>(ve, vr, B, n, nseg, n_valid, part, s); break;
    case 4: wave_launch<E, 4, EstT>(ve, vr, B, n, nseg, n_valid, part, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
template <typename EstT>
static hipError_t wave_e(const WaveView& ve, const WaveView& vr, int B, int E, int R, long long n, int nseg,
                         const int* n_valid, double* part, hipStream_t s) {
  switch (E) {
    case 1: return wave_r<1, EstT>(ve, vr, B, R, n, nseg, n_valid, part, s);
    case 2: return wave_r<2, EstT>(ve, vr, B, R, n, nseg, n_valid, part, s);
    case 3: return wave_r<3, EstT>(ve, vr, B, R, n, nseg, n_valid, part, s);
    case 4: return wave_r<4, EstT>(ve, vr, B, R, n, nseg, n_valid, part, s);
    case 5: return wave_r<5, EstT>(ve, vr, B, R, n, nseg, n_valid, part, s);
    default: return hipErrorInvalidValue;
  }
}

long long score_wave_segments(long long n) { return (n + SCORE_SEG - 1) / SCORE_SEG; }

// a view takes 16-byte loads when its samples are contiguous and every (item, source) row starts 16-byte aligned
static int wave_vec(const SigView& v) {
  const long long per = v.i16 ? 8 : 4;
  return v.st == 1 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0 && v.sb % per == 0 && v.ss % per == 0;
}

hipError_t launch_score_wave(const SigView& est, const SigView& ref, int B, int E, int R, long long n, const int* n_valid,
                             double* part, double* stats, hipStream_t s) {
  const int nseg = (int)score_wave_segments(n);
  const WaveView ve = {est, wave_vec(est)}, vr = {ref, wave_vec(ref)};
  const hipError_t e = est.i16 ? wave_e<int16_t>(ve, vr, B, E, R, n, nseg, n_valid, part, s)
                               : wave_e<float>(ve, vr, B, E, R, n, nseg, n_valid, part, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_wave_fold_k, dim3(B), dim3(128), 0, s, part, nseg, E, R, sig_unit(est), stats);
  return hipGetLastError();
}

// ---- spectral criterion ---------------------------------------------------------------------------------------------
// grid (F, items), 256 threads over the frames.  p.a = the estimates, p.b = the references ((item, f, source, t) addressing).
// Each of the three terms is formed in float32 the way the training criterion forms it (products and sums rounded one by
// one, no contraction; |r| = hypotf as torch.abs of a complex64) and added in double.
template <int E, int R>
__global__ __launch_bounds__(256) void score_spec_k(const PitArgs p, double* part) {
  __shared__ double s_tmp[4][E * R];
  const int f = blockIdx.x, b = blockIdx.y;
  const long long oa = (long long)b * p.a.sb + (long long)f * p.a.sf;
  const long long ob = (long long)b * p.b.sb + (long long)f * p.b.sf;
  double d[E * R];
#pragma unroll
  for (int i = 0; i < E * R; ++i) d[i] = 0.0;
  for (int t = threadIdx.x; t < p.T; t += 256) {
    const long long ia = oa + (long long)t * p.a.st, ib = ob + (long long)t * p.b.st;
    float er[E], ei[E], em[E], rr[R], ri[R], rm[R];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      er[i] = p.a.re[ia + i * p.a.sm];
      ei[i] = p.a.im[ia + i * p.a.sm];
      em[i] = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(er[i], er[i]), __fmul_rn(ei[i], ei[i])), 1e-8f));
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      rr[j] = p.b.re[ib + j * p.b.sm];
      ri[j] = p.b.im[ib + j * p.b.sm];
      rm[j] = hypotf(rr[j], ri[j]);
    }
#pragma unroll
    for (int i = 0; i < E; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j)
        d[i * R + j] += ((double)fabsf(er[i] - rr[j]) + (double)fabsf(ei[i] - ri[j])) + (double)fabsf(em[i] - rm[j]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < E * R; ++i) {
    double v = d[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) s_tmp[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < E * R) {
    const int i = threadIdx.x;
    part[((long long)b * gridDim.x + f) * (E * R) + i] = (s_tmp[0][i] + s_tmp[1][i]) + (s_tmp[2][i] + s_tmp[3][i]);
  }
}

// grid (items), 64 threads.  pair [item][E][R]; with perm != nullptr (E == R = S): perm[item][i] = p(i) of the permutation
// with the least sum_i pair[i][p(i)] (itertools order, first minimum), upit[item] = that sum
__global__ __launch_bounds__(64) void score_spec_fold_k(const double* part, int F, int E, int R, double* pair, int* perm,
                                                        double* upit) {
  __shared__ double s_d[5 * 4];
  const int b = blockIdx.x, ER = E * R;
  if ((int)threadIdx.x < ER) {
    const double* q = part + (long long)b * F * ER + threadIdx.x;
    double a = 0.0;
    for (int f = 0; f < F; ++f) a += q[(long long)f * ER];             // fixed order: bin 0, 1, ...
    s_d[threadIdx.x] = a;
    pair[(long long)b * ER + threadIdx.x] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0 || (!perm && !upit)) return;
  const int S = R;
  int cur[4], best[4];
  for (int k = 0; k < S; ++k) { cur[k] = k; best[k] = k; }
  double cbest = 0.0;
  bool first = true;
  for (;;) {
    double c = 0.0;
    for (int k = 0; k < S; ++k) c += s_d[k * S + cur[k]];
    if (first || c < cbest) {
      cbest = c; first = false;
      for (int k = 0; k < S; ++k) best[k] = cur[k];
    }
    int a = S - 2;                                                     // next lexicographic permutation
    while (a >= 0 && cur[a] > cur[a + 1]) --a;
    if (a < 0) break;
    int b2 = S - 1;
    while (cur[b2] < cur[a]) --b2;
    { const int t = cur[a]; cur[a] = cur[b2]; cur[b2] = t; }
    for (int lo = a + 1, hi = S - 1; lo < hi; ++lo, --hi) { const int t = cur[lo]; cur[lo] = cur[hi]; cur[hi] = t; }
  }
  if (perm)
    for (int k = 0; k < S; ++k) perm[b * S + k] = best[k];
  if (upit) upit[b] = cbest;
}

template <int E>
static hipError_t spec_r(const PitArgs& p, int R, double* part, hipStream_t s) {
  const dim3 g(p.F, p.B);
  switch (R) {
    case 1: hipLaunchKernelGGL((score_spec_k<E, 1>), g, dim3(256), 0, s, p, part); break;
    case 2: hipLaunchKernelGGL((score_spec_k<E, 2>), g, dim3(256), 0, s, p, part); break;
    case 3: hipLaunchKernelGGL((score_spec_k<E, 3>), g, dim3(256), 0, s, p, part); break;
    case 4: hipLaunchKernelGGL((score_spec_k<E, 4>), g, dim3(256), 0, s, p, part); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_score_spec(const PitArgs& p, int E, int R, double* part, double* pair, int* perm, double* upit,
                             hipStream_t s) {
  hipError_t e;
  switch (E) {
    case 1: e = spec_r<1>(p, R, part, s); break;
    case 2: e = spec_r<2>(p, R, part, s); break;
    case 3: e = spec_r<3>(p, R, part, s); break;
    case 4: e = spec_r<4>(p, R, part, s); break;
    case 5: e = spec_r<5>(p, R, part, s); break;
    default: return hipErrorInvalidValue;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_spec_fold_k, dim3(p.B), dim3(64), 0, s, part, p.F, E, R, pair, perm, upit);
  return hipGetLastError();
}

}  // namespace mn
