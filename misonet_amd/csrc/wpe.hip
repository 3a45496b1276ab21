// WPE dereverberation (Nakatani et al. 2010; Yoshioka & Nakatani 2012) on the device: C ABI misonet_wpe / misonet_wpe_debug in
// net.hip; the definition is restated in NumPy in tests/wpe_ref.py.
//
// Per (item b, bin f), independent of every other.  With N = M taps and the stacked vector s[t] = [z[t]; y[t]] of order
// K = N + M, z[(k M + m), t] = y[m, t - delay - k]:
//
//   wpe_in_k    Y [B, M, T, F] -> Yt [B, F, M, T] (and the DNN power [B, T, F] float32 -> pw [B, F, T] float64) through a
//               32 x 32 LDS tile: both sides coalesced; every bin then owns M contiguous rows of T
//   wpe_bin_k   one workgroup of 8 waves per bin, for every iteration:
//                 p[t] = mean_m |x[m, t]|^2 (x = y - G^H z from the filter of the iteration before, float64, never stored),
//                 w[t] = 1 / max(p[t], power_floor max_t p[t]);
//                 the real Gram matrix of [Re s; Im s] (2 K rows, 16 x 16 tiles, lower half) on v_mfma_f64_16x16x4_f64 with T
//                 tiled through LDS and w folded into the B operand: its blocks give the lower triangle of
//                 R = sum_t w z z^H and, as M extra ROWS below it, P^H = sum_t w y z^H;
//                 Cholesky in LDS on the K x N panel -- the extra rows leave it as (L^-1 P)^H, the forward substitution is
//                 free -- and one backward substitution turns them into G^H;
//               after the last iteration x = y - G^H z is rounded to complex64 once and written over Yt, T tiles in
//               descending order (a tile reads only frames at or below its own)
//   wpe_out_k   Yt -> out [B, M, T, F]
//
// Every sum runs in a fixed order, nothing is accumulated with atomics and a bin never looks at another one: the result of an
// item is bit-reproducible and does not depend on the batch it sits in or on its position there.  A bin whose Cholesky meets a
// pivot that is not finite or not > 0 (the all-zero bin: w infinite, R NaN) is passed through: Yt is left as it is,
// fail[b, f] = 1, its filter reads 0.
#include "kernels.hpp"

namespace mn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int WPE_TT = 64;            // frames per LDS tile: 75 KB of LDS at M = 6, 10 taps -- two workgroups per CU
constexpr int WPE_THREADS = 512;      // 8 waves
constexpr int WPE_WAVES = WPE_THREADS / 64;
constexpr int WPE_SLOTS = 9;          // 16 x 16 tiles per wave: ceil(66 / 8) at the largest 2 K = 176

__host__ __device__ inline long long wpe_align(long long x) { return (x + 255) & ~255LL; }

// workspace: fail int [B F] | G c128 [B F][N][M] | pw f64 [B F][T] | Yt c64 [B F][M][T]  (the first two do not move with T)
struct WpeWs { long long fail, g, pw, yt, total; };
__host__ __device__ inline WpeWs wpe_ws(int B, int M, int T, int F, int taps) {
  WpeWs w;
  const long long bins = (long long)B * F;
  w.fail = 0;
  w.g = wpe_align(bins * 4);
  w.pw = wpe_align(w.g + bins * M * taps * M * 16);
  w.yt = wpe_align(w.pw + bins * T * 8);
  w.total = wpe_align(w.yt + bins * M * T * 8);
  return w;
}
long long wpe_ws_bytes(int B, int M, int T, int F, int taps) { return wpe_ws(B, M, T, F, taps).total; }

// ---- the two transposes ---------------------------------------------------------------------------------------------
// grid (ceil(F / 32), ceil(T / 32), planes), 256 threads (32 x 8).  Plane r of src is [T][F]; it lands at
// dst + (r / M) * db + (r % M) * dm + f * df + t
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void wpe_in_k(const TI* src, TO* dst, int M, int T, int F, long long db, long long dm,
                                                long long df) {
  __shared__ TI tile[32][33];
  const int f0 = blockIdx.x * 32, t0 = blockIdx.y * 32, r = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const TI* s = src + (long long)r * T * F;
  for (int i = ty; i < 32; i += 8)
    if (t0 + i < T && f0 + tx < F) tile[i][tx] = s[(long long)(t0 + i) * F + f0 + tx];
  __syncthreads();
  TO* d = dst + (long long)(r / M) * db + (long long)(r % M) * dm;
  for (int i = ty; i < 32; i += 8)
    if (f0 + i < F && t0 + tx < T) {
      const TI v = tile[tx][i];
      if constexpr (sizeof(TI) == sizeof(TO)) d[(long long)(f0 + i) * df + t0 + tx] = v;
      else d[(long long)(f0 + i) * df + t0 + tx] = (TO)v;
    }
}

// grid as wpe_in_k: Yt [B][F][M][T] -> out [B][M][T][F]
__global__ __launch_bounds__(256) void wpe_out_k(const float2* yt, float2* out, int M, int T, int F) {
  __shared__ float2 tile[32][33];
  const int f0 = blockIdx.x * 32, t0 = blockIdx.y * 32, r = blockIdx.z;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float2* s = yt + (long long)(r / M) * F * M * T + (long long)(r % M) * T;
  for (int i = ty; i < 32; i += 8)
    if (f0 + i < F && t0 + tx < T) tile[i][tx] = s[(long long)(f0 + i) * M * T + t0 + tx];
  __syncthreads();
  float2* d = out + (long long)r * T * F;
  for (int i = ty; i < 32; i += 8)
    if (t0 + i < T && f0 + tx < F) d[(long long)(t0 + i) * F + f0 + tx] = tile[tx][i];
}

// ---- one bin --------------------------------------------------------------------------------------------------------
struct WpeArgs {
  float2* yt;
  double* pw;
  double* g;
  int* fail;
  int M, T, taps, delay, iters, has_power;
  double diag_load, power_floor;
};

// LDS of wpe_bin_k, in bytes from the start of the dynamic block
struct WpeLds { int S, col, wt, px, red, zwin, ywin, zero, total, zp; };
__host__ __device__ inline WpeLds wpe_lds(int M, int taps) {
  const int N = M * taps, K = N + M;
  WpeLds l;
  l.zp = (WPE_TT + taps - 1) | 1;                                      // row pitch of the z window, in floats (odd)
  l.S = 0;                                                             // double2 [K][N]
  l.col = l.S + K * N * 16;                                            // double2 [K]
  l.wt = l.col + K * 16;                                               // double [TT]
  l.px = l.wt + WPE_TT * 8;                                            // double [M][TT]
  l.red = l.px + M * WPE_TT * 8;                                       // double [WAVES]
  l.zwin = l.red + WPE_WAVES * 8;                                      // float [2 M][zp]: frames t0 - delay - (taps - 1) ...
  l.ywin = l.zwin + 2 * M * l.zp * 4;                                  // float [2 M][TT]: frames t0 ...
  l.zero = l.ywin + 2 * M * WPE_TT * 4;                                // float [TT] of zeros: the rows past 2 K
  l.total = l.zero + WPE_TT * 4;
  return l;
}

// where row rho of [Re s; Im s] starts in the staged windows (float index from zwin), so that + tl gives frame t0 + tl
__device__ __forceinline__ int wpe_row_off(int rho, int M, int N, int K, int taps, const WpeLds& l) {
  if (rho >= 2 * K) return (l.zero - l.zwin) / 4;
  const int part = rho >= K ? 1 : 0, q = rho - part * K;
  if (q < N) {
    const int k = q / M, m = q - k * M;
    return (part * M + m) * l.zp + (taps - 1 - k);
  }
  return (l.ywin - l.zwin) / 4 + (part * M + (q - N)) * WPE_TT;
}

// tile number tau, counted row by row over the lower half, -> (I, J); an unused slot reads as tile 0
__device__ __forceinline__ void wpe_tile(int tau, int ntiles, int& I, int& J) {
  if (tau >= ntiles) tau = 0;
  I = 0;
  while (tau > I) { tau -= I + 1; ++I; }
  J = tau;
}

// stages the frames of tile t0: the z window (when asked) and the y window, real parts in rows [0, M), imaginary in [M, 2 M)
__device__ __forceinline__ void wpe_stage(const float2* y, int M, int T, int taps, int delay, int t0, bool want_z, float* zwin,
                                          float* ywin, int zp) {
  if (want_z) {
    const int zl = WPE_TT + taps - 1, tb = t0 - delay - (taps - 1);
    for (int e = threadIdx.x; e < M * zl; e += WPE_THREADS) {
      const int m = e / zl, i = e - m * zl, t = tb + i;
      float2 v = {0.f, 0.f};
      if (t >= 0 && t < T) v = y[(long long)m * T + t];
      zwin[m * zp + i] = v.x;
      zwin[(M + m) * zp + i] = v.y;
    }
  }
  for (int e = threadIdx.x; e < M * WPE_TT; e += WPE_THREADS) {
    const int m = e / WPE_TT, i = e - m * WPE_TT, t = t0 + i;
    float2 v = {0.f, 0.f};
    if (t < T) v = y[(long long)m * T + t];
    ywin[m * WPE_TT + i] = v.x;
    ywin[(M + m) * WPE_TT + i] = v.y;
  }
}

// x = y - G^H z for the staged tile (G^H = rows N .. K - 1 of S; x = y without a filter).  pw[t] = mean_m |x|^2, or, with
// store, x rounded to complex64 over y.  Ends behind a barrier: the windows may be staged again.
__device__ __forceinline__ void wpe_apply_tile(float2* y, double* pwb, int M, int N, int T, int taps, int t0, bool filt,
                                               bool store, const double2* S, const float* zwin, const float* ywin, int zp,
                                               double* px) {
  for (int e = threadIdx.x; e < M * WPE_TT; e += WPE_THREADS) {
    const int m = e / WPE_TT, tl = e - m * WPE_TT;
    double xr = (double)ywin[m * WPE_TT + tl], xi = (double)ywin[(M + m) * WPE_TT + tl];
    if (filt) {
      const double2* gh = S + (long long)(N + m) * N;
      double sr = 0.0, si = 0.0;
      for (int k = 0; k < taps; ++k) {
        const int zo = tl + taps - 1 - k;
        for (int mm = 0; mm < M; ++mm) {
          const double2 c = gh[k * M + mm];
          const double zr = (double)zwin[mm * zp + zo], zi = (double)zwin[(M + mm) * zp + zo];
          sr += c.x * zr - c.y * zi;
          si += c.x * zi + c.y * zr;
        }
      }
      xr -= sr;
      xi -= si;
    }
    if (store) {
      if (t0 + tl < T) y[(long long)m * T + t0 + tl] = make_float2((float)xr, (float)xi);
    } else {
      px[m * WPE_TT + tl] = xr * xr + xi * xi;
    }
  }
  __syncthreads();
  if (!store) {
    if (threadIdx.x < WPE_TT && t0 + (int)threadIdx.x < T) {
      double p = 0.0;
      for (int m = 0; m < M; ++m) p += px[m * WPE_TT + threadIdx.x];   // fixed order: microphone 0, 1, ...
      pwb[t0 + threadIdx.x] = p / (double)M;
    }
    __syncthreads();
  }
}

// grid (B F bins), 512 threads, wpe_lds(M, taps).total bytes of dynamic LDS
__global__ __launch_bounds__(WPE_THREADS) void wpe_bin_k(const WpeArgs a) {
  extern __shared__ __align__(16) unsigned char wpe_smem[];
  const int M = a.M, T = a.T, taps = a.taps, N = M * taps, K = N + M;
  const WpeLds l = wpe_lds(M, taps);
  double2* S = reinterpret_cast<double2*>(wpe_smem + l.S);
  double2* col = reinterpret_cast<double2*>(wpe_smem + l.col);
  double* wt = reinterpret_cast<double*>(wpe_smem + l.wt);
  double* px = reinterpret_cast<double*>(wpe_smem + l.px);
  double* red = reinterpret_cast<double*>(wpe_smem + l.red);
  float* zwin = reinterpret_cast<float*>(wpe_smem + l.zwin);
  float* ywin = reinterpret_cast<float*>(wpe_smem + l.ywin);
  float* zero = reinterpret_cast<float*>(wpe_smem + l.zero);
  const int zp = l.zp;
  const long long bin = blockIdx.x;
  float2* y = a.yt + bin * M * T;
  double* pwb = a.pw + bin * T;
  double2* gout = reinterpret_cast<double2*>(a.g) + bin * N * M;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int ntile_t = (T + WPE_TT - 1) / WPE_TT;

  if (tid < WPE_TT) zero[tid] = 0.f;
  if (tid == 0) a.fail[bin] = 0;

  // the 16 x 16 tiles (I >= J) of the 2 K x 2 K Gram matrix this wave owns: tile number wave + 8 slot, counted row by row
  const int NT = (2 * K + 15) / 16, ntiles = NT * (NT + 1) / 2;
  int offA[WPE_SLOTS], offB[WPE_SLOTS];
#pragma unroll
  for (int s = 0; s < WPE_SLOTS; ++s) {
    int I, J;
    wpe_tile(wave + WPE_WAVES * s, ntiles, I, J);
    offA[s] = wpe_row_off(16 * I + lr, M, N, K, taps, l) + lg;         // A[i = lr][k = lg], B[k = lg][j = lr]
    offB[s] = wpe_row_off(16 * J + lr, M, N, K, taps, l) + lg;
  }
  const int nslots = __builtin_amdgcn_readfirstlane(wave < ntiles ? (ntiles - 1 - wave) / WPE_WAVES + 1 : 0);

  bool failed = false;
#pragma unroll 1
  for (int it = 0; it < a.iters && !failed; ++it) {
    // ---- p[t] into pw (the first iteration of a DNN-WPE call finds it there) and its maximum
    if (it > 0 || !a.has_power) {
#pragma unroll 1
      for (int tt = 0; tt < ntile_t; ++tt) {
        __syncthreads();
        wpe_stage(y, M, T, taps, a.delay, tt * WPE_TT, it > 0, zwin, ywin, zp);
        __syncthreads();
        wpe_apply_tile(y, pwb, M, N, T, taps, tt * WPE_TT, it > 0, false, S, zwin, ywin, zp, px);
      }
    }
    __syncthreads();
    double pm = 0.0;
    for (int t = tid; t < T; t += WPE_THREADS) pm = fmax(pm, pwb[t]);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) pm = fmax(pm, __shfl_xor(pm, k, 64));
    if (lane == 0) red[wave] = pm;
    __syncthreads();
    pm = red[0];
#pragma unroll
    for (int k = 1; k < WPE_WAVES; ++k) pm = fmax(pm, red[k]);
    const double thr = a.power_floor * pm;

    // ---- the Gram matrix of [Re s; Im s], w folded into B
    d4 acc[WPE_SLOTS];
#pragma unroll
    for (int s = 0; s < WPE_SLOTS; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int tt = 0; tt < ntile_t; ++tt) {
      const int t0 = tt * WPE_TT;
      __syncthreads();
      wpe_stage(y, M, T, taps, a.delay, t0, true, zwin, ywin, zp);
      if (tid < WPE_TT) wt[tid] = t0 + tid < T ? 1.0 / fmax(pwb[t0 + tid], thr) : 0.0;
      __syncthreads();
#pragma unroll 1
      for (int k4 = 0; k4 < WPE_TT; k4 += 4) {                         // the loads of a step first, then its MFMAs
        const double wv = wt[k4 + lg];
        float av[WPE_SLOTS], bv[WPE_SLOTS];
#pragma unroll
        for (int s = 0; s < WPE_SLOTS; ++s)
          if (s < nslots) {                                            // wave-uniform
            av[s] = zwin[offA[s] + k4];
            bv[s] = zwin[offB[s] + k4];
          }
#pragma unroll
        for (int s = 0; s < WPE_SLOTS; ++s)
          if (s < nslots) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[s], (double)bv[s] * wv, acc[s], 0, 0, 0);
      }
    }

    // ---- the K x N panel [R; P^H] from the blocks of the Gram matrix.  Element (rho_i, rho_j), rho = part K + q:
    //   phase 0  Re Re:  S[qi][qj].re  = g        phase 2  Im Re, qi >= qj:  S[qi][qj].im  = g
    //   phase 1  Im Im:  S[qi][qj].re += g        phase 3  Im Re, qi <= qj:  S[qj][qi].im -= g
    // every component is written by one lane per phase; C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
      __syncthreads();
#pragma unroll
      for (int s = 0; s < WPE_SLOTS; ++s)
        if (s < nslots) {
          int I, J;
          wpe_tile(wave + WPE_WAVES * s, ntiles, I, J);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ri = 16 * I + lg + 4 * r, rj = 16 * J + lr;
            if (ri < rj || ri >= 2 * K) continue;
            const int pi = ri >= K, pj = rj >= K, qi = ri - pi * K, qj = rj - pj * K;
            const double g = acc[s][r];
            if (ph == 0 && !pi && !pj && qj < N) S[qi * N + qj].x = g;
            if (ph == 1 && pi && pj && qj < N) S[qi * N + qj].x += g;
            if (ph == 2 && pi && !pj && qi >= qj && qj < N) S[qi * N + qj].y = g;
            if (ph == 3 && pi && !pj && qi <= qj && qi < N) S[qj * N + qi].y -= g;
          }
        }
    }
    __syncthreads();
    if (a.diag_load != 0.0) {
      if (tid == 0) {
        double tr = 0.0;
        for (int i = 0; i < N; ++i) tr += S[i * N + i].x;
        red[0] = a.diag_load * tr / (double)N;
      }
      __syncthreads();
      if (tid < N) S[tid * N + tid].x += red[0];
      __syncthreads();
    }

    // ---- Cholesky of the panel, column by column; every thread sees the same pivot
    const int tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
    for (int c = 0; c < N; ++c) {
      const double piv = S[c * N + c].x;
      if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) { failed = true; break; }
      const double d = sqrt(piv);
      __syncthreads();                                                 // the pivot is read before the column is rewritten
      for (int i = c + tid; i < K; i += WPE_THREADS) {
        double2 v = S[i * N + c];
        if (i == c) v = make_double2(d, 0.0);
        else { v.x /= d; v.y /= d; }
        col[i] = v;
        S[i * N + c] = v;
      }
      __syncthreads();
      for (int j = c + 1 + tx; j < N; j += 16) {
        const double2 lj = col[j];
        for (int i = c + 1 + ty; i < K; i += WPE_THREADS / 16)
          if (i >= j) {
            const double2 li = col[i];
            double2 v = S[i * N + j];
            v.x -= li.x * lj.x + li.y * lj.y;                          // l_i conj(l_j)
            v.y -= li.y * lj.x - li.x * lj.y;
            S[i * N + j] = v;
          }
      }
      __syncthreads();
    }
    if (failed) break;

    // ---- G^H L = X, columns from the last one; rows N .. K - 1 end as G^H
#pragma unroll 1
    for (int j = N - 1; j >= 0; --j) {
      if (tid < M) {
        double2 v = S[(N + tid) * N + j];
        const double d = S[j * N + j].x;
        v.x /= d;
        v.y /= d;
        S[(N + tid) * N + j] = v;
      }
      __syncthreads();
      for (int e = tid; e < M * j; e += WPE_THREADS) {
        const int m = e / j, jj = e - m * j;
        const double2 gm = S[(N + m) * N + j], lv = S[j * N + jj];
        double2 v = S[(N + m) * N + jj];
        v.x -= gm.x * lv.x - gm.y * lv.y;
        v.y -= gm.x * lv.y + gm.y * lv.x;
        S[(N + m) * N + jj] = v;
      }
      __syncthreads();
    }
  }

  if (failed) {                                                        // uniform: Yt stays the observation
    if (tid == 0) a.fail[bin] = 1;
    for (int e = tid; e < N * M; e += WPE_THREADS) gout[e] = make_double2(0.0, 0.0);
    return;
  }
  for (int e = tid; e < N * M; e += WPE_THREADS) {                     // G[j][m] = conj(G^H[m][j])
    const int j = e / M, m = e - j * M;
    const double2 v = S[(N + m) * N + j];
    gout[e] = make_double2(v.x, -v.y);
  }
#pragma unroll 1
  for (int tt = ntile_t - 1; tt >= 0; --tt) {
    __syncthreads();
    wpe_stage(y, M, T, taps, a.delay, tt * WPE_TT, true, zwin, ywin, zp);
    __syncthreads();
    wpe_apply_tile(y, pwb, M, N, T, taps, tt * WPE_TT, true, true, S, zwin, ywin, zp, px);
  }
}

hipError_t launch_wpe(const void* mix, const float* power, int B, int M, int T, int F, int taps, int delay, int iters,
                      double diag_load, double power_floor, void* out, void* ws, hipStream_t s) {
  const WpeWs w = wpe_ws(B, M, T, F, taps);
  char* base = reinterpret_cast<char*>(ws);
  WpeArgs a;
  a.yt = reinterpret_cast<float2*>(base + w.yt);
  a.pw = reinterpret_cast<double*>(base + w.pw);
  a.g = reinterpret_cast<double*>(base + w.g);
  a.fail = reinterpret_cast<int*>(base + w.fail);
  a.M = M; a.T = T; a.taps = taps; a.delay = delay; a.iters = iters; a.has_power = power != nullptr;
  a.diag_load = diag_load; a.power_floor = power_floor;
  const dim3 tg((F + 31) / 32, (T + 31) / 32, B * M);
  hipLaunchKernelGGL((wpe_in_k<float2, float2>), tg, dim3(256), 0, s, reinterpret_cast<const float2*>(mix), a.yt, M, T, F,
                     (long long)F * M * T, (long long)T, (long long)M * T);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (power) {
    hipLaunchKernelGGL((wpe_in_k<float, double>), dim3(tg.x, tg.y, B), dim3(256), 0, s, power, a.pw, 1, T, F, (long long)F * T,
                       0LL, (long long)T);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const int lds = wpe_lds(M, taps).total;
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wpe_bin_k), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(wpe_bin_k, dim3(B * F), dim3(WPE_THREADS), lds, s, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(wpe_out_k, tg, dim3(256), 0, s, a.yt, reinterpret_cast<float2*>(out), M, T, F);
  return hipGetLastError();
}

hipError_t launch_wpe_debug(const void* ws, int B, int M, int F, int taps, void* g, int* fail, hipStream_t s) {
  const WpeWs w = wpe_ws(B, M, 2, F, taps);
  const char* base = reinterpret_cast<const char*>(ws);
  const long long bins = (long long)B * F;
  if (g) {
    hipError_t e = hipMemcpyAsync(g, base + w.g, bins * M * taps * M * 16, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  if (fail) return hipMemcpyAsync(fail, base + w.fail, bins * 4, hipMemcpyDeviceToDevice, s);
  return hipSuccess;
}

}  // namespace mn
