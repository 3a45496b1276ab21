// Streaming polyphase resampler (include/misonet.h misonet_resample_stream*): resample.hip's definition, fed in
// blocks.  A stream that has seen N samples per channel has emitted the outputs m < e(N) whose last input j_hi(m) has arrived,
//
//   e(N) = 0 where N p - 1 - Lh < 0, else floor((N p - 1 - Lh) / q) + 1,
//
// and carries its last C = floor(2 Lh / p) samples as float32 [B][M][C], aligned to the end of the stream and zero where the
// stream has not begun (an int16 sample is carried as its integer value).  A call computes y[m] = sum_j x[j] g[m q - j p + Lh] for
// its own outputs with x[j] read from "carried tail ++ block": the same float64 sum over the same j in ascending order as
// resample_k, rounded once -- the bits of the offline kernel.  (The carried zeros in front of sample 0 enter the sums of the first
// outputs, where resample_k clips at 0: a sum that starts at +0.0 is never -0.0, so adding +-0.0 terms moves no bit.)
//
// Everything in a launch is RELATIVE to the block: inputs are jr = j - N in [-C, n_new), outputs i = m - e(N), and the tap of
// (i, jr) is D + i q - jr p + Lh with D = e(N) q - N p: in [-Lh, 0] before the stream emits, in (-Lh - 1, -Lh - 1 + q] after.
// N itself never reaches the device, so a captured call replays over the following blocks of the same length whenever that
// length is a multiple of q (D and the counts repeat).  The index arithmetic is 64-bit: i q and jr p pass 2^31 for a block of
// 2^28 samples.
//
// resample_stream_k: one workgroup owns RSS_TILE = 32 consecutive outputs of one item for all of its M <= 16 channels.  The
// offline tile (256) leaves a 64-sample call at the model rate as one quarter-filled workgroup per item; 32 gives such a call two
// workgroups per item and a 1024-sample call 32, and keeps KMAX = ceil(32 M / 256) at 1 up to 8 channels.  A lone small workgroup
// is bound by the latency of its loads, not by their number, so (a) the whole tap table is staged into LDS once per workgroup when
// it fits (max(p, q) <= 204: every ratio between 8, 16, 32, 48 kHz and 48 <-> 44.1 kHz), and read from global memory otherwise
// (44.1 <-> 16 kHz: 8821 taps), and (b) the walk is unrolled by four so the loads of four steps are in flight under one wait.
// Work item (output i / M, channel i % M) as in resample_k: neighbouring lanes read neighbouring LDS words and share the tap.
//
// resample_tail_k, behind it on the same stream: the new tail, the last C samples of tail ++ block, one workgroup per
// (channel, item).  n_new >= C: a copy out of the block.  Otherwise the tail moves left by n_new in place in ascending chunks of
// 256 (read a chunk, barrier, write it: a chunk's writes lie below every later read), then the block fills the end.
#include "kernels.hpp"
#include "resample_round.hpp"

namespace mn {

constexpr int RSS_TILE = 32;             // output samples per workgroup
constexpr int RSS_THREADS = 256;
constexpr int RSS_LDS = 4096;            // float32 words of sample staging (16 KB)
constexpr int RSS_TAPS = 4096;           // float64 taps held in LDS (32 KB); a longer table is read from global memory

int resample_stream_tile() { return RSS_TILE; }

int resample_stream_carry(int p, int q) { return 2 * resample_half_len(p, q) / p; }

long long resample_stream_emitted(long long N, int p, int q) {
  const long long a = N * p - 1 - resample_half_len(p, q);
  return a < 0 ? 0 : a / q + 1;
}

__device__ __forceinline__ long long rss_floor_div(long long a, long long b) {      // b > 0
  const long long d = a / b;
  return d * b > a ? d - 1 : d;
}

struct RssView { long long sb, sc, st; int i16; };

// s += x[0] g[t] + x[M] g[t - p] + ... (n terms), term after term: resample_k's expression, the loads of four steps together
template <class G>
__device__ __forceinline__ double rss_walk(double s, const float* x, int M, const G* g, int t, int p, int n) {
#pragma unroll 4
  for (int r = 0; r < n; ++r) {
    s += (double)*x * g[t];
    x += M;
    t -= p;
  }
  return s;
}

// grid (ceil(n_out / RSS_TILE), items), RSS_THREADS threads; KMAX = ceil(RSS_TILE M / RSS_THREADS) sums per thread.
// tail [items][M][C] (nullptr where C == 0); D = e(N) q - N p; outputs i in [0, n_out) go to dst element i along dv.st
template <int KMAX>
__global__ __launch_bounds__(RSS_THREADS) void resample_stream_k(const void* src, RssView sv, int M, long long n_new,
                                                                const float* tail, int C, long long D, int p, int q, int Lh,
                                                                const double* g, long long n_out, void* dst, RssView dv) {
  __shared__ float s_x[RSS_LDS];
  __shared__ double s_g[RSS_TAPS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long i0 = (long long)blockIdx.x * RSS_TILE;
  const long long i_end = i0 + RSS_TILE < n_out ? i0 + RSS_TILE : n_out;       // outputs [i0, i_end) are this tile's
  const int items = (int)(i_end - i0) * M;
  const bool taps_lds = 2 * Lh + 1 <= RSS_TAPS;                                 // block-uniform
  if (taps_lds)
    for (int e = tid; e <= 2 * Lh; e += RSS_THREADS) s_g[e] = g[e];             // the first barrier of the walk covers it

  double acc[KMAX];
  long long jlo[KMAX], jhi[KMAX];                                               // the inputs under each output's taps, relative
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    acc[k] = 0.0;
    jlo[k] = 0;
    jhi[k] = -1;
    const int i = k * RSS_THREADS + tid;
    if (i < items) {
      const long long c = D + (i0 + i / M) * q;
      jlo[k] = -rss_floor_div(Lh - c, p);                                       // ceil((c - Lh) / p), not below -C
      if (jlo[k] < -C) jlo[k] = -C;
      jhi[k] = rss_floor_div(c + Lh, p);                                        // floor((c + Lh) / p), not above n_new - 1
      if (jhi[k] > n_new - 1) jhi[k] = n_new - 1;
    }
  }
  {
    const long long c0 = D + i0 * q, c1 = D + (i_end - 1) * q;
    long long J0 = -rss_floor_div(Lh - c0, p), J1 = rss_floor_div(c1 + Lh, p);
    if (J0 < -C) J0 = -C;
    if (J1 > n_new - 1) J1 = n_new - 1;
    const int CH = RSS_LDS / M;                                                 // samples per chunk
    const bool chan_fast = sv.sc <= sv.st;                                      // which axis of the source neighbours in memory
    const long long base = (long long)b * sv.sb;
    const float* tl = tail + (long long)b * M * C + C;                          // tl[c C + jr], jr in [-C, 0)
    for (long long cj = J0; cj <= J1; cj += CH) {
      const int cn = (int)(J1 - cj + 1 < CH ? J1 - cj + 1 : CH);
      for (int e = tid; e < cn * M; e += RSS_THREADS) {
        int jl, c;
        if (chan_fast) { jl = e / M; c = e - jl * M; } else { c = e / cn; jl = e - c * cn; }
        const long long jr = cj + jl;
        float v;
        if (jr < 0) {
          v = tl[(long long)c * C + jr];
        } else {
          const long long at = base + jr * sv.st + (long long)c * sv.sc;
          v = sv.i16 ? (float)reinterpret_cast<const int16_t*>(src)[at] : reinterpret_cast<const float*>(src)[at];
        }
        s_x[jl * M + c] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const long long a = jlo[k] > cj ? jlo[k] : cj;
        const long long z = jhi[k] < cj + cn - 1 ? jhi[k] : cj + cn - 1;
        if (a <= z) {
          const int i = k * RSS_THREADS + tid;
          const int ml = i / M, c = i - ml * M;
          const int t = (int)(D + (i0 + ml) * q - a * p + Lh);                  // tap index of jr = a; p less for every next one
          const float* x = s_x + (int)(a - cj) * M + c;
          const int n = (int)(z - a) + 1;
          acc[k] = taps_lds ? rss_walk(acc[k], x, M, s_g, t, p, n) : rss_walk(acc[k], x, M, g, t, p, n);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int i = k * RSS_THREADS + tid;
    if (i >= items) continue;
    const int ml = i / M, c = i - ml * M;
    const double y = sv.i16 ? acc[k] * (1.0 / 32767.0) : acc[k];                // the int16 rule: scaled once, after the sum
    const long long at = (long long)b * dv.sb + (long long)c * dv.sc + (i0 + ml) * dv.st;
    if (dv.i16) reinterpret_cast<short*>(dst)[at] = rs_to_i16(y);
    else reinterpret_cast<float*>(dst)[at] = (float)y;
  }
}

// grid (M, items), RSS_THREADS threads, C >= 1, n_new >= 1: tail <- the last C samples of tail ++ block
__global__ __launch_bounds__(RSS_THREADS) void resample_tail_k(const void* src, RssView sv, int M, long long n_new, float* tail,
                                                              int C) {
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float* tl = tail + ((long long)b * M + c) * C;
  const long long base = (long long)b * sv.sb + (long long)c * sv.sc;
  const int keep = n_new >= C ? 0 : C - (int)n_new;                            // carried samples that stay, moved to the front
  if (keep > 0) {
    const int sh = C - keep;                                                    // = n_new
    for (int k0 = 0; k0 < keep; k0 += RSS_THREADS) {
      const int k = k0 + tid;
      float v = 0.f;
      if (k < keep) v = tl[k + sh];
      __syncthreads();                                                          // every read of the chunk before any write of it
      if (k < keep) tl[k] = v;
    }
  }
  const long long first = n_new - (C - keep);                                   // the block's samples [first, n_new) follow
  for (int k = keep + tid; k < C; k += RSS_THREADS) {
    const long long at = base + (first + (k - keep)) * sv.st;
    tl[k] = sv.i16 ? (float)reinterpret_cast<const int16_t*>(src)[at] : reinterpret_cast<const float*>(src)[at];
  }
}

// One call of the stream: n_out outputs (resample_stream_k, when n_out > 0), then, with `update`, the tail after the block's
// n_new samples (resample_tail_k, when C > 0 and n_new > 0).
hipError_t launch_resample_stream(const void* src, int src_i16, const long long* ss, int B, int M, long long n_new, long long D,
                                  long long n_out, int update, int p, int q, const double* taps, void* dst, int dst_i16,
                                  const long long* ds, float* tail, hipStream_t s) {
  if (B < 1 || B > 65535 || M < 1 || M > RS_MAX_CH || n_new < 0 || n_out < 0 || p < 1 || q < 1) return hipErrorInvalidValue;
  const long long tiles = (n_out + RSS_TILE - 1) / RSS_TILE;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  const RssView sv = {ss[0], ss[1], ss[2], src_i16}, dv = {ds[0], ds[1], ds[2], dst_i16};
  const int Lh = resample_half_len(p, q), C = resample_stream_carry(p, q);
  if (n_out > 0) {
    const dim3 grid((unsigned)tiles, (unsigned)B), block(RSS_THREADS);
    if (M <= RSS_THREADS / RSS_TILE)
      hipLaunchKernelGGL(resample_stream_k<1>, grid, block, 0, s, src, sv, M, n_new, tail, C, D, p, q, Lh, taps, n_out, dst, dv);
    else
      hipLaunchKernelGGL(resample_stream_k<2>, grid, block, 0, s, src, sv, M, n_new, tail, C, D, p, q, Lh, taps, n_out, dst, dv);
  }
  if (update && C > 0 && n_new > 0)
    hipLaunchKernelGGL(resample_tail_k, dim3((unsigned)M, (unsigned)B), dim3(RSS_THREADS), 0, s, src, sv, M, n_new, tail, C);
  return hipGetLastError();
}

}  // namespace mn
