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
//                 the weighted Gram matrix of the stacked vector by the scheme of stacked_gram.hpp, of which the first N
//                 columns are kept: the lower triangle of R = sum_t w z z^H and, as M extra ROWS below it,
//                 P^H = sum_t w y z^H;
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
#include "stacked_gram.hpp"

namespace mn {

// workspace: fail int [B F] | G c128 [B F][N][M] | pw f64 [B F][T] | Yt c64 [B F][M][T]  (the first two do not move with T)
struct WpeWs { long long fail, g, pw, yt, total; };
__host__ __device__ inline WpeWs wpe_ws(int B, int M, int T, int F, int taps) {
  WpeWs w;
  const long long bins = (long long)B * F;
  w.fail = 0;
  w.g = sg_align(bins * 4);
  w.pw = sg_align(w.g + bins * M * taps * M * 16);
  w.yt = sg_align(w.pw + bins * T * 8);
  w.total = sg_align(w.yt + bins * M * T * 8);
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
  l.zp = sg_zpitch(taps);
  l.S = 0;                                                             // double2 [K][N]
  l.col = l.S + K * N * 16;                                            // double2 [K]
  l.wt = l.col + K * 16;                                               // double [TT]
  l.px = l.wt + SG_TT * 8;                                             // double [M][TT]
  l.red = l.px + M * SG_TT * 8;                                        // double [WAVES]
  l.zwin = l.red + SG_WAVES * 8;                                       // float [2 M][zp]: frames t0 - delay - (taps - 1) ...
  l.ywin = l.zwin + 2 * M * l.zp * 4;                                  // float [2 M][TT]: frames t0 ...
  l.zero = l.ywin + 2 * M * SG_TT * 4;                                 // float [TT] of zeros: the rows past 2 K
  l.total = l.zero + SG_TT * 4;
  return l;
}

// x = y - G^H z for the staged tile (G^H = rows N .. K - 1 of S; x = y without a filter).  pw[t] = mean_m |x|^2, or, with
// store, x rounded to complex64 over y.  Ends behind a barrier: the windows may be staged again.
__device__ __forceinline__ void wpe_apply_tile(float2* y, double* pwb, int M, int N, int T, int taps, int t0, bool filt,
                                               bool store, const double2* S, const float* zwin, const float* ywin, int zp,
                                               double* px) {
  for (int e = threadIdx.x; e < M * SG_TT; e += SG_THREADS) {
    const int m = e / SG_TT, tl = e - m * SG_TT;
    double xr = (double)ywin[m * SG_TT + tl], xi = (double)ywin[(M + m) * SG_TT + tl];
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
      px[m * SG_TT + tl] = xr * xr + xi * xi;
    }
  }
  __syncthreads();
  if (!store) {
    if (threadIdx.x < SG_TT && t0 + (int)threadIdx.x < T) {
      double p = 0.0;
      for (int m = 0; m < M; ++m) p += px[m * SG_TT + threadIdx.x];    // fixed order: microphone 0, 1, ...
      pwb[t0 + threadIdx.x] = p / (double)M;
    }
    __syncthreads();
  }
}

// grid (B F bins), 512 threads, wpe_lds(M, taps).total bytes of dynamic LDS
__global__ __launch_bounds__(SG_THREADS) void wpe_bin_k(const WpeArgs a) {
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
  const int tid = threadIdx.x;
  const int ntile_t = (T + SG_TT - 1) / SG_TT;
  const SgWin win = {l.zwin, l.ywin, l.zero, zp};
  const auto load = [=](int m, int t) { return y[(long long)m * T + t]; };

  if (tid < SG_TT) zero[tid] = 0.f;
  if (tid == 0) a.fail[bin] = 0;

  SgTiles g;
  sg_tiles_init(g, M, N, K, taps, win);

  bool failed = false;
#pragma unroll 1
  for (int it = 0; it < a.iters && !failed; ++it) {
    // ---- p[t] into pw (the first iteration of a DNN-WPE call finds it there) and its maximum
    if (it > 0 || !a.has_power) {
#pragma unroll 1
      for (int tt = 0; tt < ntile_t; ++tt) {
        __syncthreads();
        sg_stage(load, M, T, taps, a.delay, tt * SG_TT, it > 0, zwin, ywin, zp);
        __syncthreads();
        wpe_apply_tile(y, pwb, M, N, T, taps, tt * SG_TT, it > 0, false, S, zwin, ywin, zp, px);
      }
    }
    __syncthreads();
    double pm = 0.0;
    for (int t = tid; t < T; t += SG_THREADS) pm = fmax(pm, pwb[t]);
    const double thr = a.power_floor * sg_block_max(pm, red);

    // ---- the Gram matrix of [Re s; Im s], w folded into B
    sg_gram_zero(g);
#pragma unroll 1
    for (int tt = 0; tt < ntile_t; ++tt) {
      const int t0 = tt * SG_TT;
      __syncthreads();
      sg_stage(load, M, T, taps, a.delay, t0, true, zwin, ywin, zp);
      if (tid < SG_TT) wt[tid] = t0 + tid < T ? 1.0 / fmax(pwb[t0 + tid], thr) : 0.0;
      __syncthreads();
      sg_gram_tile(g, zwin, wt, [](int) {});
    }

    // ---- the K x N panel [R; P^H] from the blocks of the Gram matrix, its Cholesky
    sg_panel(g, K, N, S);
    __syncthreads();
    if (a.diag_load != 0.0) {
      sg_diag_load(S, N, a.diag_load, red);
      __syncthreads();
    }
    if (!sg_cholesky(S, K, N, col)) { failed = true; break; }

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
      for (int e = tid; e < M * j; e += SG_THREADS) {
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
    for (int e = tid; e < N * M; e += SG_THREADS) gout[e] = make_double2(0.0, 0.0);
    return;
  }
  for (int e = tid; e < N * M; e += SG_THREADS) {                      // G[j][m] = conj(G^H[m][j])
    const int j = e / M, m = e - j * M;
    const double2 v = S[(N + m) * N + j];
    gout[e] = make_double2(v.x, -v.y);
  }
#pragma unroll 1
  for (int tt = ntile_t - 1; tt >= 0; --tt) {
    __syncthreads();
    sg_stage(load, M, T, taps, a.delay, tt * SG_TT, true, zwin, ywin, zp);
    __syncthreads();
    wpe_apply_tile(y, pwb, M, N, T, taps, tt * SG_TT, true, true, S, zwin, ywin, zp, px);
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
  hipLaunchKernelGGL(wpe_bin_k, dim3(B * F), dim3(SG_THREADS), lds, s, a);
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
