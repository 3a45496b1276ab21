// Polyphase resampler (include/misonet.h misonet_resample*): scipy.signal.resample_poly's definition for
// any rational rate p / q = fs_out / fs_in with max(p, q) <= 1024, every channel on its own:
//
//   Lh = 10 max(p, q),   h = firwin(2 Lh + 1, 1 / max(p, q), window = ("kaiser", 5.0)),   g = p h
//   y[m] = sum_j x[j] g[m q - j p + Lh],   j ascending over 0 <= j < n with the tap index inside [0, 2 Lh],   0 <= m < ceil(n p / q)
//
// (p = q = 1: Lh = 0, g = {1}: a copy).  The taps are built on the host in float64; the sum is float64 in that order and is
// rounded once, to float32 or -- x 32767, round to nearest even, saturated to [-32768, 32767] -- to int16.  An int16 input sample
// stands for itself / 32767, scaled once after the sum (the int16 rule of score.hip).  No atomics: bit-reproducible, and an output
// depends on nothing but its own channel of its own item.
//
// One workgroup owns RS_TILE consecutive output samples of one item for all of its M channels.  The input span the tile needs is
// walked in chunks of RS_LDS / M samples, each staged into LDS as float32 [sample][channel] (an int16 sample converts exactly)
// with loads that follow the fastest axis of the source, so that the time-major layout [n][M] of a wav file and the channel-major
// [M][n] are both read coalesced; a chunk is as long as the LDS allows, so at 1 / 3 a tile is one chunk and at 1 / 1024 it is many.
// Work item i = k 256 + thread of the tile is (output i / M, channel i % M): neighbouring lanes read neighbouring LDS words, share
// the tap (one address per output) and keep their sums in registers across the chunks, which keeps j ascending.
#include "kernels.hpp"
#include "resample_round.hpp"

#include <cmath>
#include <numeric>
#include <vector>

namespace mn {

constexpr int RS_TILE = 256;            // output samples per workgroup
constexpr int RS_THREADS = 256;
constexpr int RS_LDS = 12288;           // float32 words of staging (48 KB)

int resample_tile() { return RS_TILE; }

bool resample_ratio(long long fs_in, long long fs_out, int* p, int* q) {
  if (fs_in < 1 || fs_out < 1 || fs_in > 0x7fffffffLL || fs_out > 0x7fffffffLL) return false;
  const long long g = std::gcd(fs_in, fs_out);
  const long long pp = fs_out / g, qq = fs_in / g;
  if (pp > RS_MAX_RATE || qq > RS_MAX_RATE) return false;
  *p = (int)pp;
  *q = (int)qq;
  return true;
}

int resample_half_len(int p, int q) { return (p == 1 && q == 1) ? 0 : 10 * (p > q ? p : q); }

long long resample_len(long long n, int p, int q) { return (n * p + q - 1) / q; }

// g[0 .. 2 Lh]: SciPy's firwin step for step -- the ideal low-pass cutoff sinc(cutoff k), the Kaiser window of beta 5, the
// division by the sum (unit gain at 0 Hz) -- times p
void resample_build_taps(int p, int q, double* g) {
  const int Lh = resample_half_len(p, q);
  if (Lh == 0) { g[0] = 1.0; return; }
  const double pi = 3.14159265358979323846, beta = 5.0;
  const double cutoff = 1.0 / (p > q ? p : q), i0b = sig_i0(beta);
  double sum = 0.0, comp = 0.0;                                        // a compensated sum: up to 20481 terms of both signs
  for (int i = 0; i <= 2 * Lh; ++i) {
    const double k = (double)(i - Lh);
    const double a = pi * (cutoff * k);
    const double sinc = (i == Lh) ? 1.0 : std::sin(a) / a;
    const double u = k / Lh;
    const double r = 1.0 - u * u;
    g[i] = cutoff * sinc * (sig_i0(beta * std::sqrt(r > 0.0 ? r : 0.0)) / i0b);
    const double t = sum + g[i];
    comp += std::fabs(sum) >= std::fabs(g[i]) ? (sum - t) + g[i] : (g[i] - t) + sum;
    sum = t;
  }
  sum += comp;
  for (int i = 0; i <= 2 * Lh; ++i) g[i] = g[i] / sum * p;
}

struct RsView { long long sb, sc, st; int i16; };

// grid (ceil(n_out / RS_TILE), items), RS_THREADS threads; KMAX = ceil(RS_TILE M / RS_THREADS) sums per thread
template <int KMAX>
__global__ __launch_bounds__(RS_THREADS) void resample_k(const void* src, RsView sv, int M, long long n, const int* n_valid,
                                                         int p, int q, int Lh, const double* g, long long n_out, void* dst,
                                                         RsView dv) {
  __shared__ float s_x[RS_LDS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long m0 = (long long)blockIdx.x * RS_TILE;
  const long long nv = sig_nv(n_valid, b, n);
  const long long len = (nv * p + q - 1) / q;                          // this item's own output length
  const long long m_end = m0 + RS_TILE < n_out ? m0 + RS_TILE : n_out; // outputs [m0, m_end) are this tile's
  const long long m_live = m_end < len ? m_end : len;                  // ... and [m0, m_live) of them are not zeros
  const int items = (int)(m_end - m0) * M;

  double acc[KMAX];
  long long jlo[KMAX], jhi[KMAX];                                      // the inputs under each output's taps
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    acc[k] = 0.0;
    jlo[k] = 0;
    jhi[k] = -1;
    const int i = k * RS_THREADS + tid;
    const long long m = m0 + i / M;
    if (i < items && m < m_live) {
      const long long c = m * q;
      jlo[k] = c - Lh <= 0 ? 0 : (c - Lh + p - 1) / p;                 // ceil((m q - Lh) / p), not below 0
      jhi[k] = (c + Lh) / p;                                           // floor((m q + Lh) / p), not above nv - 1
      if (jhi[k] > nv - 1) jhi[k] = nv - 1;
    }
  }
  if (m_live > m0) {                                                   // block-uniform
    const long long c0 = m0 * q, c1 = (m_live - 1) * q;
    const long long J0 = c0 - Lh <= 0 ? 0 : (c0 - Lh + p - 1) / p;
    long long J1 = (c1 + Lh) / p;
    if (J1 > nv - 1) J1 = nv - 1;
    const int CH = RS_LDS / M;                                         // samples per chunk
    const bool chan_fast = sv.sc <= sv.st;                             // which axis of the source neighbours in memory
    const long long base = (long long)b * sv.sb;
    for (long long cj = J0; cj <= J1; cj += CH) {
      const int cn = (int)(J1 - cj + 1 < CH ? J1 - cj + 1 : CH);
      for (int e = tid; e < cn * M; e += RS_THREADS) {
        int jl, c;
        if (chan_fast) { jl = e / M; c = e - jl * M; } else { c = e / cn; jl = e - c * cn; }
        const long long at = base + (cj + jl) * sv.st + (long long)c * sv.sc;
        s_x[jl * M + c] = sv.i16 ? (float)reinterpret_cast<const int16_t*>(src)[at] : reinterpret_cast<const float*>(src)[at];
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const long long a = jlo[k] > cj ? jlo[k] : cj;
        const long long z = jhi[k] < cj + cn - 1 ? jhi[k] : cj + cn - 1;
        if (a <= z) {
          const int i = k * RS_THREADS + tid;
          const int ml = i / M, c = i - ml * M;
          int t = (int)((m0 + ml) * q - a * p + Lh);                   // tap index of j = a; p less for every next j
          const float* x = s_x + (int)(a - cj) * M + c;
          double s = acc[k];
          for (int r = (int)(z - a); r >= 0; --r) {
            s += (double)*x * g[t];
            x += M;
            t -= p;
          }
          acc[k] = s;
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int i = k * RS_THREADS + tid;
    if (i >= items) continue;
    const int ml = i / M, c = i - ml * M;
    const double y = sv.i16 ? acc[k] * (1.0 / 32767.0) : acc[k];      // the int16 rule: scaled once, after the sum
    const long long at = (long long)b * dv.sb + (long long)c * dv.sc + (m0 + ml) * dv.st;
    if (dv.i16) reinterpret_cast<short*>(dst)[at] = rs_to_i16(y);
    else reinterpret_cast<float*>(dst)[at] = (float)y;
  }
}

hipError_t launch_resample(const void* src, int src_i16, const long long* ss, int B, int M, long long n, const int* n_valid, int p,
                           int q, const double* taps, void* dst, int dst_i16, const long long* ds, hipStream_t s) {
  if (B < 1 || B > 65535 || M < 1 || M > RS_MAX_CH || n < 1 || p < 1 || q < 1) return hipErrorInvalidValue;
  const long long n_out = resample_len(n, p, q);
  const long long tiles = (n_out + RS_TILE - 1) / RS_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const RsView sv = {ss[0], ss[1], ss[2], src_i16}, dv = {ds[0], ds[1], ds[2], dst_i16};
  const dim3 grid((unsigned)tiles, (unsigned)B), block(RS_THREADS);
  const int Lh = resample_half_len(p, q);
#define RS_LAUNCH(K) \
  hipLaunchKernelGGL(resample_k<K>, grid, block, 0, s, src, sv, M, n, n_valid, p, q, Lh, taps, n_out, dst, dv)
  if (M <= 1) RS_LAUNCH(1);
  else if (M <= 2) RS_LAUNCH(2);
  else if (M <= 4) RS_LAUNCH(4);
  else if (M <= 8) RS_LAUNCH(8);
  else RS_LAUNCH(16);
#undef RS_LAUNCH
  return hipGetLastError();
}

}  // namespace mn
