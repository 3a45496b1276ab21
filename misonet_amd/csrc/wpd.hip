// WPD convolutional beamformer (Nakatani & Kinoshita 2019, in the mask-based form of Zhang, Boeddeker et al. 2020 that ESPnet
// calls "wpd") on the device: C ABI misonet_wpd / misonet_wpd_debug / misonet_pipeline_set_wpd in api_array.hip and
// api_pipeline.hip; the definition is restated in NumPy in tests/wpd_ref.py.
//
// Per (item b, speaker s, bin f), independent of every other: Y = mix[b, f] [M, T], S = the source estimate [M, T].  With
// N = M taps, z[(k M + m), t] = y[m, t - delay - k] and the stacked vector of order K = N + M:
//
//   wpd_bin_k   one workgroup of 8 waves per (b, s, f):
//                 p[t] = mean_m |S[m, t]|^2, w[t] = 1 / max(p[t], power_floor max_t p[t])  (a first sweep over S for the maximum);
//                 the real Gram matrix of [Re s; Im s] (2 K rows, 16 x 16 tiles, lower half) on v_mfma_f64_16x16x4_f64 with T
//                 tiled through LDS and w folded into the B operand -- the scheme of wpe_bin_k, here with the stacking order
//                 s = [z; y] INSIDE the kernel (the interface order is [y; z]) -- and beside it, on the last wave, the
//                 unweighted Gram tile of [Re S; Im S] (2 M <= 16 rows: one tile), which gives Phi_s = S S^H / T;
//                 R = sum_t w s s^H (+ diag_load tr(R) / K I), K x K, Cholesky R = L L^H in LDS;
//                 L X = Phibar: with the order [z; y] only the last M x M block of L takes part (rows < N of X stay 0);
//                 L^H A = X for the M right-hand sides, tr(A), wbar = A[:, ref_ch] / tr(A);
//                 a last sweep over T: out[t] = wbar^H s[t], rounded to complex64 once, on the store
//
// Every sum runs in a fixed order, nothing is accumulated with atomics and a workgroup never looks at another one: the result
// is bit-reproducible and depends neither on B, nor on S, nor on the position in the batch.  A (b, s, f) whose Cholesky meets a
// pivot that is not finite or not > 0 (the all-zero bin or source: w infinite, R not finite), or whose tr(A) is not finite or 0,
// FAILS: wbar = 0, out = 0, fail = 1.  Nothing is clamped.
//
// Limits: 2 <= M <= 8, taps >= 1, delay >= 1, K = M (taps + 1) <= 88 -- the order the Gram scheme reaches with 9 accumulator
// tiles per wave; the K x K factor (121 KB at K = 88), the right-hand sides and the windows take 156 KB of the 160 KB of LDS at
// M = 8, 10 taps, the largest case -- and T > delay + taps - 1.  The host checks them before any launch.
#include "kernels.hpp"

namespace mn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int WPD_TT = 64;            // frames per LDS tile
constexpr int WPD_THREADS = 512;      // 8 waves
constexpr int WPD_WAVES = WPD_THREADS / 64;
constexpr int WPD_SLOTS = 9;          // 16 x 16 tiles per wave: ceil(66 / 8) at the largest 2 K = 176
constexpr int WPD_LDS_LIMIT = 160 * 1024;

__host__ __device__ inline long long wpd_align(long long x) { return (x + 255) & ~255LL; }

// workspace: fail int [B S F] | wbar c128 [B S F][K] (interface order [y; z])
struct WpdWs { long long fail, w, total; };
__host__ __device__ inline WpdWs wpd_ws(int B, int S, int F, int M, int taps) {
  WpdWs w;
  const long long bins = (long long)B * S * F;
  w.fail = 0;
  w.w = wpd_align(bins * 4);
  w.total = wpd_align(w.w + bins * M * (taps + 1) * 16);
  return w;
}
long long wpd_ws_bytes(int B, int S, int F, int M, int taps) { return wpd_ws(B, S, F, M, taps).total; }

// LDS of wpd_bin_k, in bytes from the start of the dynamic block
struct WpdLds { int R, col, X, wb, wt, red, part, zwin, ywin, swin, zero, total, zp; };
__host__ __device__ inline WpdLds wpd_lds(int M, int taps) {
  const int N = M * taps, K = N + M;
  WpdLds l;
  l.zp = (WPD_TT + taps - 1) | 1;                                      // row pitch of the z window, in floats (odd)
  l.R = 0;                                                             // double2 [K][K], lower triangle
  l.col = l.R + K * K * 16;                                            // double2 [K]
  l.X = l.col + K * 16;                                                // double2 [M][K]: the right-hand sides, one per row
  l.wb = l.X + M * K * 16;                                             // double2 [K]: wbar in the kernel's order [z; y]
  l.wt = l.wb + K * 16;                                                // double [TT]
  l.red = l.wt + WPD_TT * 8;                                           // double [WAVES]
  l.part = l.red + WPD_WAVES * 8;                                      // double2 [WAVES][TT] of the apply; before it double [16][16]
  l.zwin = l.part + WPD_WAVES * WPD_TT * 16;                           // float [2 M][zp]: frames t0 - delay - (taps - 1) ...
  l.ywin = l.zwin + 2 * M * l.zp * 4;                                  // float [2 M][TT]: frames t0 ...
  l.swin = l.ywin + 2 * M * WPD_TT * 4;                                // float [2 M][TT]: the source estimate
  l.zero = l.swin + 2 * M * WPD_TT * 4;                                // float [TT] of zeros: the rows past 2 K / 2 M
  l.total = l.zero + WPD_TT * 4;
  return l;
}
int wpd_lds_bytes(int M, int taps) { return wpd_lds(M, taps).total; }

// where row rho of [Re s; Im s], s = [z; y], starts in the staged windows (float index from zwin), so that + tl gives frame t0 + tl
__device__ __forceinline__ int wpd_row_off(int rho, int M, int N, int K, int taps, const WpdLds& l) {
  if (rho >= 2 * K) return (l.zero - l.zwin) / 4;
  const int part = rho >= K ? 1 : 0, q = rho - part * K;
  if (q < N) {
    const int k = q / M, m = q - k * M;
    return (part * M + m) * l.zp + (taps - 1 - k);
  }
  return (l.ywin - l.zwin) / 4 + (part * M + (q - N)) * WPD_TT;
}

// tile number tau, counted row by row over the lower half, -> (I, J); an unused slot reads as tile 0
__device__ __forceinline__ void wpd_tile(int tau, int ntiles, int& I, int& J) {
  if (tau >= ntiles) tau = 0;
  I = 0;
  while (tau > I) { tau -= I + 1; ++I; }
  J = tau;
}

// source estimate of aligned speaker `spk` at microphone m: pointers to its frame row for bin f (as launch_mvdr reads it)
__device__ __forceinline__ void wpd_src_row(const WpdArgs& a, int b, int f, int m, int spk, const float*& re, const float*& im,
                                            int& st) {
  if (a.est) {
    const int n = b * a.M + m;
    const int q = a.sel ? a.sel[n * a.S + spk] : spk;
    const long long plane = (long long)a.F * a.Tp;
    const float* base = a.est + (long long)n * a.est_bstride + (long long)f * a.Tp;
    re = base + (long long)q * plane;
    im = base + (long long)(a.S + q) * plane;
    st = 1;
  } else {
    const long long off = (long long)b * a.src.sb + (long long)f * a.src.sf + (long long)m * a.src.sm;
    re = a.src.re + off;
    im = a.src.im + off;
    st = a.src.st;
  }
}

// stages the frames of tile t0: the z and y windows of the observation, real parts in rows [0, M), imaginary in [M, 2 M), and
// (when asked) the source estimate in the same form
__device__ __forceinline__ void wpd_stage(const WpdArgs& a, int b, int f, int spk, int t0, bool want_s, float* zwin, float* ywin,
                                          float* swin, int zp) {
  const int M = a.M, T = a.T, taps = a.taps;
  const long long yoff = (long long)b * a.mix.sb + (long long)f * a.mix.sf;
  const float* yre = a.mix.re + yoff;
  const float* yim = a.mix.im + yoff;
  const long long yst = a.mix.st;
  const int zl = WPD_TT + taps - 1, tb = t0 - a.delay - (taps - 1);
  for (int e = threadIdx.x; e < M * zl; e += WPD_THREADS) {
    const int m = e / zl, i = e - m * zl, t = tb + i;
    float vr = 0.f, vi = 0.f;
    if (t >= 0 && t < T) {
      vr = yre[(long long)m * a.mix.sm + t * yst];
      vi = yim[(long long)m * a.mix.sm + t * yst];
    }
    zwin[m * zp + i] = vr;
    zwin[(M + m) * zp + i] = vi;
  }
  for (int e = threadIdx.x; e < M * WPD_TT; e += WPD_THREADS) {
    const int m = e / WPD_TT, i = e - m * WPD_TT, t = t0 + i;
    float vr = 0.f, vi = 0.f;
    if (t < T) {
      vr = yre[(long long)m * a.mix.sm + t * yst];
      vi = yim[(long long)m * a.mix.sm + t * yst];
    }
    ywin[m * WPD_TT + i] = vr;
    ywin[(M + m) * WPD_TT + i] = vi;
  }
  if (want_s) {
    for (int e = threadIdx.x; e < M * WPD_TT; e += WPD_THREADS) {
      const int m = e / WPD_TT, i = e - m * WPD_TT, t = t0 + i;
      float vr = 0.f, vi = 0.f;
      if (t < T) {
        const float *sre, *sim;
        int sst;
        wpd_src_row(a, b, f, m, spk, sre, sim, sst);
        vr = sre[(long long)t * sst];
        vi = sim[(long long)t * sst];
      }
      swin[m * WPD_TT + i] = vr;
      swin[(M + m) * WPD_TT + i] = vi;
    }
  }
}

// grid (F, B, S), 512 threads, wpd_lds(M, taps).total bytes of dynamic LDS
__global__ __launch_bounds__(WPD_THREADS) void wpd_bin_k(const WpdArgs a, const COut out, int* fail_out, double2* w_out) {
  extern __shared__ __align__(16) unsigned char wpd_smem[];
  const int M = a.M, T = a.T, taps = a.taps, N = M * taps, K = N + M;
  const WpdLds l = wpd_lds(M, taps);
  double2* R = reinterpret_cast<double2*>(wpd_smem + l.R);
  double2* col = reinterpret_cast<double2*>(wpd_smem + l.col);
  double2* X = reinterpret_cast<double2*>(wpd_smem + l.X);
  double2* wb = reinterpret_cast<double2*>(wpd_smem + l.wb);
  double* wt = reinterpret_cast<double*>(wpd_smem + l.wt);
  double* red = reinterpret_cast<double*>(wpd_smem + l.red);
  double2* part = reinterpret_cast<double2*>(wpd_smem + l.part);
  double* gs = reinterpret_cast<double*>(wpd_smem + l.part);            // the Gram tile of the source, before the apply
  float* zwin = reinterpret_cast<float*>(wpd_smem + l.zwin);
  float* ywin = reinterpret_cast<float*>(wpd_smem + l.ywin);
  float* swin = reinterpret_cast<float*>(wpd_smem + l.swin);
  float* zero = reinterpret_cast<float*>(wpd_smem + l.zero);
  const int zp = l.zp;
  const int f = blockIdx.x, b = blockIdx.y, spk = blockIdx.z;
  const long long bin = ((long long)b * a.S + spk) * a.F + f;
  double2* wg = w_out + bin * K;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int ntile_t = (T + WPD_TT - 1) / WPD_TT;
  const long long oo = (long long)b * out.ob + (long long)spk * out.os + (long long)f * out.of;
  float* ore = out.re + oo;
  float* oim = out.im + oo;

  if (tid < WPD_TT) zero[tid] = 0.f;

  // ---- the maximum of p[t] = mean_m |S[m, t]|^2 (the same arithmetic as below, on the same float32 values)
  double pm = 0.0;
  for (int t = tid; t < T; t += WPD_THREADS) {
    double p = 0.0;
    for (int m = 0; m < M; ++m) {                                      // fixed order: microphone 0, 1, ...
      const float *sre, *sim;
      int sst;
      wpd_src_row(a, b, f, m, spk, sre, sim, sst);
      const double xr = (double)sre[(long long)t * sst], xi = (double)sim[(long long)t * sst];
      p = fma(xr, xr, p);
      p = fma(xi, xi, p);
    }
    pm = fmax(pm, p / (double)M);
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) pm = fmax(pm, __shfl_xor(pm, k, 64));
  if (lane == 0) red[wave] = pm;
  __syncthreads();
  pm = red[0];
#pragma unroll
  for (int k = 1; k < WPD_WAVES; ++k) pm = fmax(pm, red[k]);
  const double thr = a.power_floor * pm;

  // the 16 x 16 tiles (I >= J) of the 2 K x 2 K Gram matrix this wave owns: tile number wave + 8 slot, counted row by row
  const int NT = (2 * K + 15) / 16, ntiles = NT * (NT + 1) / 2;
  int offA[WPD_SLOTS], offB[WPD_SLOTS];
#pragma unroll
  for (int s = 0; s < WPD_SLOTS; ++s) {
    int I, J;
    wpd_tile(wave + WPD_WAVES * s, ntiles, I, J);
    offA[s] = wpd_row_off(16 * I + lr, M, N, K, taps, l) + lg;         // A[i = lr][k = lg], B[k = lg][j = lr]
    offB[s] = wpd_row_off(16 * J + lr, M, N, K, taps, l) + lg;
  }
  const int nslots = __builtin_amdgcn_readfirstlane(wave < ntiles ? (ntiles - 1 - wave) / WPD_WAVES + 1 : 0);
  // the one tile of [Re S; Im S]: row lr of it, both operands (the last wave has the fewest tiles of the other kind)
  const int offS = (lr < 2 * M ? (l.swin - l.zwin) / 4 + lr * WPD_TT : (l.zero - l.zwin) / 4) + lg;
  const bool src_wave = wave == WPD_WAVES - 1;                         // wave-uniform

  // ---- the Gram matrix of [Re s; Im s], w folded into B; the Gram tile of the source estimate
  d4 acc[WPD_SLOTS];
#pragma unroll
  for (int s = 0; s < WPD_SLOTS; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  d4 accs = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * WPD_TT;
    __syncthreads();
    wpd_stage(a, b, f, spk, t0, true, zwin, ywin, swin, zp);
    __syncthreads();
    if (tid < WPD_TT) {
      double p = 0.0;
      for (int m = 0; m < M; ++m) {
        const double xr = (double)swin[m * WPD_TT + tid], xi = (double)swin[(M + m) * WPD_TT + tid];
        p = fma(xr, xr, p);
        p = fma(xi, xi, p);
      }
      wt[tid] = t0 + tid < T ? 1.0 / fmax(p / (double)M, thr) : 0.0;
    }
    __syncthreads();
#pragma unroll 1
    for (int k4 = 0; k4 < WPD_TT; k4 += 4) {                           // the loads of a step first, then its MFMAs
      const double wv = wt[k4 + lg];
      float av[WPD_SLOTS], bv[WPD_SLOTS];
#pragma unroll
      for (int s = 0; s < WPD_SLOTS; ++s)
        if (s < nslots) {                                              // wave-uniform
          av[s] = zwin[offA[s] + k4];
          bv[s] = zwin[offB[s] + k4];
        }
      if (src_wave) {
        const double sv = (double)zwin[offS + k4];
        accs = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, sv, accs, 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < WPD_SLOTS; ++s)
        if (s < nslots) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[s], (double)bv[s] * wv, acc[s], 0, 0, 0);
    }
  }

  // ---- R (lower triangle) from the blocks of the Gram matrix.  Element (rho_i, rho_j), rho = part K + q:
  //   phase 0  Re Re:  R[qi][qj].re  = g        phase 2  Im Re, qi >= qj:  R[qi][qj].im  = g
  //   phase 1  Im Im:  R[qi][qj].re += g        phase 3  Im Re, qi <= qj:  R[qj][qi].im -= g
  // every component is written by one lane per phase; C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
#pragma unroll 1
  for (int ph = 0; ph < 4; ++ph) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < WPD_SLOTS; ++s)
      if (s < nslots) {
        int I, J;
        wpd_tile(wave + WPD_WAVES * s, ntiles, I, J);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ri = 16 * I + lg + 4 * r, rj = 16 * J + lr;
          if (ri < rj || ri >= 2 * K) continue;
          const int pi = ri >= K, pj = rj >= K, qi = ri - pi * K, qj = rj - pj * K;
          const double g = acc[s][r];
          if (ph == 0 && !pi && !pj) R[qi * K + qj].x = g;
          if (ph == 1 && pi && pj) R[qi * K + qj].x += g;
          if (ph == 2 && pi && !pj && qi >= qj) R[qi * K + qj].y = g;
          if (ph == 3 && pi && !pj && qi <= qj) R[qj * K + qi].y -= g;
        }
      }
  }
  if (src_wave) {
#pragma unroll
    for (int r = 0; r < 4; ++r) gs[(lg + 4 * r) * 16 + lr] = accs[r];
  }
  __syncthreads();
  // Phibar as the right-hand sides: X[c][N + i] = Phi_s[i][c] = (S S^H)[i][c] / T from its lower triangle (Hermitian by
  // construction, a real diagonal); rows < N are 0.  Re = G[i][j] + G[M + i][M + j], Im = G[M + i][j] - G[M + j][i]
  for (int e = tid; e < M * K; e += WPD_THREADS) {
    const int c = e / K, r = e - c * K;
    double2 v = make_double2(0.0, 0.0);
    if (r >= N) {
      const int i = r - N, hi = i >= c ? i : c, lo = i >= c ? c : i;
      const double invT = 1.0 / (double)T;
      v.x = (gs[hi * 16 + lo] + gs[(M + hi) * 16 + M + lo]) * invT;
      v.y = hi == lo ? 0.0 : (gs[(M + hi) * 16 + lo] - gs[(M + lo) * 16 + hi]) * invT;
      if (i < c) v.y = -v.y;
    }
    X[e] = v;
  }
  if (a.diag_load != 0.0) {
    if (tid == 0) {
      double tr = 0.0;
      for (int i = 0; i < K; ++i) tr += R[i * K + i].x;
      red[0] = a.diag_load * tr / (double)K;
    }
    __syncthreads();
    if (tid < K) R[tid * K + tid].x += red[0];
  }
  __syncthreads();

  // ---- Cholesky of R, column by column; every thread sees the same pivot
  bool failed = false;
  const int tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
  for (int c = 0; c < K; ++c) {
    const double piv = R[c * K + c].x;
    if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) { failed = true; break; }
    const double d = sqrt(piv);
    __syncthreads();                                                   // the pivot is read before the column is rewritten
    for (int i = c + tid; i < K; i += WPD_THREADS) {
      double2 v = R[i * K + c];
      if (i == c) v = make_double2(d, 0.0);
      else { v.x /= d; v.y /= d; }
      col[i] = v;
      R[i * K + c] = v;
    }
    __syncthreads();
    for (int j = c + 1 + tx; j < K; j += 16) {
      const double2 lj = col[j];
      for (int i = c + 1 + ty; i < K; i += WPD_THREADS / 16)
        if (i >= j) {
          const double2 li = col[i];
          double2 v = R[i * K + j];
          v.x -= li.x * lj.x + li.y * lj.y;                            // l_i conj(l_j)
          v.y -= li.y * lj.x - li.x * lj.y;
          R[i * K + j] = v;
        }
    }
    __syncthreads();
  }

  if (!failed) {
    // ---- L X = Phibar: the last M x M block of L only; right-hand side c on thread c
    if (tid < M) {
      double2* x = X + tid * K + N;
      for (int i = 0; i < M; ++i) {
        double2 v = x[i];
        for (int k = 0; k < i; ++k) {
          const double2 lv = R[(N + i) * K + N + k], xk = x[k];
          v.x -= lv.x * xk.x - lv.y * xk.y;
          v.y -= lv.x * xk.y + lv.y * xk.x;
        }
        const double d = R[(N + i) * K + N + i].x;
        x[i] = make_double2(v.x / d, v.y / d);
      }
    }
    __syncthreads();
    // ---- L^H A = X, rows from the last one: (L^H)[r][i] = conj(L[i][r])
#pragma unroll 1
    for (int i = K - 1; i >= 0; --i) {
      if (tid < M) {
        double2 v = X[tid * K + i];
        const double d = R[i * K + i].x;
        X[tid * K + i] = make_double2(v.x / d, v.y / d);
      }
      __syncthreads();
      for (int e = tid; e < M * i; e += WPD_THREADS) {
        const int c = e / i, r = e - c * i;
        const double2 xi = X[c * K + i], lv = R[i * K + r];
        double2 v = X[c * K + r];
        v.x -= lv.x * xi.x + lv.y * xi.y;                              // conj(l) x
        v.y -= lv.x * xi.y - lv.y * xi.x;
        X[c * K + r] = v;
      }
      __syncthreads();
    }
    // ---- tr(A): column c of A is right-hand side c, its diagonal element sits in row N + c
    if (tid == 0) {
      double tr_re = 0.0, tr_im = 0.0;
      for (int c = 0; c < M; ++c) { tr_re += X[c * K + N + c].x; tr_im += X[c * K + N + c].y; }
      red[0] = tr_re;
      red[1] = tr_im;
    }
    __syncthreads();
    const double tr_re = red[0], tr_im = red[1];
    const double big = 1.7976931348623157e308;
    if (!(fabs(tr_re) <= big) || !(fabs(tr_im) <= big) || (tr_re == 0.0 && tr_im == 0.0)) failed = true;   // uniform
    if (!failed) {
      const double den = tr_re * tr_re + tr_im * tr_im;
      for (int r = tid; r < K; r += WPD_THREADS) {
        const double2 v = X[a.ref * K + r];
        const double2 w = make_double2((v.x * tr_re + v.y * tr_im) / den, (v.y * tr_re - v.x * tr_im) / den);
        wb[r] = w;
        wg[r >= N ? r - N : M + r] = w;                                // interface order [y; z]
      }
    }
  }

  if (failed) {                                                        // uniform
    if (tid == 0) fail_out[bin] = 1;
    for (int r = tid; r < K; r += WPD_THREADS) wg[r] = make_double2(0.0, 0.0);
    for (int t = tid; t < T; t += WPD_THREADS) {
      ore[(long long)t * out.ot] = 0.f;
      oim[(long long)t * out.ot] = 0.f;
    }
    return;
  }
  if (tid == 0) fail_out[bin] = 0;

  // ---- out[t] = wbar^H s[t]: wave v adds the rows v, v + 8, ... of a frame, the eight partial sums are added in wave order
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * WPD_TT;
    __syncthreads();
    wpd_stage(a, b, f, spk, t0, false, zwin, ywin, swin, zp);
    __syncthreads();
    double sr = 0.0, si = 0.0;
    for (int r = wave; r < K; r += WPD_WAVES) {
      const double2 w = wb[r];
      double vr, vi;
      if (r < N) {
        const int k = r / M, m = r - k * M, zo = lane + taps - 1 - k;
        vr = (double)zwin[m * zp + zo];
        vi = (double)zwin[(M + m) * zp + zo];
      } else {
        vr = (double)ywin[(r - N) * WPD_TT + lane];
        vi = (double)ywin[(M + r - N) * WPD_TT + lane];
      }
      sr += w.x * vr + w.y * vi;                                       // conj(w) s
      si += w.x * vi - w.y * vr;
    }
    part[wave * WPD_TT + lane] = make_double2(sr, si);
    __syncthreads();
    if (tid < WPD_TT && t0 + tid < T) {
      double2 v = part[tid];
#pragma unroll
      for (int k = 1; k < WPD_WAVES; ++k) { v.x += part[k * WPD_TT + tid].x; v.y += part[k * WPD_TT + tid].y; }
      ore[(long long)(t0 + tid) * out.ot] = (float)v.x;
      oim[(long long)(t0 + tid) * out.ot] = (float)v.y;
    }
  }
}

hipError_t wpd_init() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&wpd_bin_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                             WPD_LDS_LIMIT);
}

hipError_t launch_wpd(const WpdArgs& a, const COut& out, void* ws, hipStream_t s) {
  const int lds = wpd_lds(a.M, a.taps).total;
  if (a.M < 2 || a.M > 8 || a.taps < 1 || a.M * (a.taps + 1) > WPD_KMAX || lds > WPD_LDS_LIMIT || a.ref < 0 || a.ref >= a.M)
    return hipErrorInvalidValue;
  const WpdWs w = wpd_ws(a.B, a.S, a.F, a.M, a.taps);
  char* base = reinterpret_cast<char*>(ws);
  hipLaunchKernelGGL(wpd_bin_k, dim3(a.F, a.B, a.S), dim3(WPD_THREADS), lds, s, a, out, reinterpret_cast<int*>(base + w.fail),
                     reinterpret_cast<double2*>(base + w.w));
  return hipGetLastError();
}

hipError_t launch_wpd_debug(const void* ws, int B, int S, int F, int M, int taps, void* wbar, int* fail, hipStream_t s) {
  const WpdWs w = wpd_ws(B, S, F, M, taps);
  const char* base = reinterpret_cast<const char*>(ws);
  const long long bins = (long long)B * S * F;
  if (wbar) {
    hipError_t e = hipMemcpyAsync(wbar, base + w.w, bins * M * (taps + 1) * 16, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return e;
  }
  if (fail) return hipMemcpyAsync(fail, base + w.fail, bins * 4, hipMemcpyDeviceToDevice, s);
  return hipSuccess;
}

}  // namespace mn
