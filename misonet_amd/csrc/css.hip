// Continuous separation of a long recording in half-overlapping windows (the "continuous speech separation" of the paper the
// reference implements, arXiv 2010.01703): the speaker order of window k is linked to window k-1 through their shared
// frames, and the windows' waveforms are joined with a raised-cosine cross-fade.  The pairwise distances of the shared
// frames are pit_dist_k / pit_pick_k (mvdr.hip) over a strided view: misonet_css_align in net.hip.
//
//   css_chain_k   P_0 = perm0 (or identity), P_k[s] = L_k[P_{k-1}[s]]: the sequential composition of the local picks
//   css_stitch_k  out[s][m] = y_k[P_k[s]][j] (k = min(K-1, m / H), j = m - kH), cross-faded with y_{k-1}[P_{k-1}[s]][H + j]
//                 over the first ov = W - H samples of every window but the first
#include "kernels.hpp"

namespace mn {

// One wave.  perm [K][S]: rows 1..K-1 hold the local picks L_k on entry, every row holds P_k on exit.  Tiles of 64 windows
// go through LDS (one coalesced load and store per tile); lane 0 composes them in window order.  perm0 may alias row 0.
template <int S>
__global__ __launch_bounds__(64) void css_chain_k(const int* perm0, int* perm, int K) {
  __shared__ int s_p[64 * S];
  const int lane = threadIdx.x;
  int prev[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int v = perm0 ? perm0[s] : s;
    prev[s] = (unsigned)v < (unsigned)S ? v : s;             // never index outside the row
  }
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    if (k < K && k > 0)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int v = perm[(long long)k * S + s];
        s_p[lane * S + s] = (unsigned)v < (unsigned)S ? v : s;
      }
    __syncthreads();
    if (lane == 0) {
      const int n = K - k0 < 64 ? K - k0 : 64;
      for (int i = 0; i < n; ++i) {
        if (k0 + i > 0) {
          int cur[S];
#pragma unroll
          for (int s = 0; s < S; ++s) cur[s] = s_p[i * S + prev[s]];
#pragma unroll
          for (int s = 0; s < S; ++s) prev[s] = cur[s];
        }
#pragma unroll
        for (int s = 0; s < S; ++s) s_p[i * S + s] = prev[s];
      }
    }
    __syncthreads();
    if (k < K)
#pragma unroll
      for (int s = 0; s < S; ++s) perm[(long long)k * S + s] = s_p[lane * S + s];
    __syncthreads();
  }
}

hipError_t launch_css_chain(const int* perm0, int* perm, int K, int S, hipStream_t s) {
  switch (S) {
    case 1: hipLaunchKernelGGL(css_chain_k<1>, dim3(1), dim3(64), 0, s, perm0, perm, K); break;
    case 2: hipLaunchKernelGGL(css_chain_k<2>, dim3(1), dim3(64), 0, s, perm0, perm, K); break;
    case 3: hipLaunchKernelGGL(css_chain_k<3>, dim3(1), dim3(64), 0, s, perm0, perm, K); break;
    case 4: hipLaunchKernelGGL(css_chain_k<4>, dim3(1), dim3(64), 0, s, perm0, perm, K); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// grid (blocks over the output samples, S).  y [K][S][W] float32 (the iSTFT of every window), perm [K][S].  Output sample
// o of speaker s is sample m = base + o of the batch (base = 0, or H when window 0 is carried over from the previous
// batch).  Lanes take consecutive samples: the y rows and the output rows are read and written in whole 256-byte runs.
// The ramp is evaluated per sample in float64 and rounded once (r = sin^2, c = cos^2 of pi (j + 1/2) / (2 ov)); the blend is
// two float32 products and one float32 sum, kept apart (no contraction), so any batching of the windows gives the same bits.
__global__ __launch_bounds__(256) void css_stitch_k(const float* y, const int* perm, int K, int S, int W, int hop,
                                                    long long base, long long n_out, short* out_i16, float* out_f32) {
  const int s = blockIdx.y;
  const int ov = W - hop;
  for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < n_out; o += 256LL * gridDim.x) {
    const long long m = base + o;
    const long long kq = m / hop;
    const int k = kq < K - 1 ? (int)kq : K - 1;
    const int j = (int)(m - (long long)k * hop);
    int p = perm[(long long)k * S + s];
    p = (unsigned)p < (unsigned)S ? p : s;
    float v = y[((long long)k * S + p) * W + j];
    if (k >= 1 && j < ov) {
      int q = perm[(long long)(k - 1) * S + s];
      q = (unsigned)q < (unsigned)S ? q : s;
      const float a = y[((long long)(k - 1) * S + q) * W + hop + j];
      const double x = 3.14159265358979323846 * (j + 0.5) / (2.0 * ov);
      const double sn = sin(x), cs = cos(x);
      const float r = (float)(sn * sn), c = (float)(cs * cs);
      v = __fadd_rn(__fmul_rn(c, a), __fmul_rn(r, v));
    }
    const long long d = (long long)s * n_out + o;
    if (out_f32) out_f32[d] = v;
    if (out_i16) out_i16[d] = (short)(int)(v * 32767.0f);                    // the truncating cast of istft_k
  }
}

hipError_t launch_css_stitch(const float* y, const int* perm, int K, int S, int W, int hop, long long base, long long n_out,
                             short* out_i16, float* out_f32, hipStream_t s) {
  long long nb = (n_out + 255) / 256;
  if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(css_stitch_k, dim3((unsigned)nb, S), dim3(256), 0, s, y, perm, K, S, W, hop, base, n_out, out_i16,
                     out_f32);
  return hipGetLastError();
}

}  // namespace mn
