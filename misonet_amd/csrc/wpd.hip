// WPD convolutional beamformer (Nakatani & Kinoshita 2019, in the mask-based form of Zhang, Boeddeker et al. 2020 that ESPnet
// calls "wpd") on the device: C ABI misonet_wpd / misonet_wpd_debug / misonet_pipeline_set_wpd in api_array.hip and
// api_pipeline.hip; the definition is restated in NumPy in tests/wpd_ref.py.
//
// Per (item b, speaker s, bin f), independent of every other: Y = mix[b, f] [M, T], S = the source estimate [M, T].  With
// N = M taps, z[(k M + m), t] = y[m, t - delay - k] and the stacked vector of order K = N + M:
//
//   wpd_bin_k   one workgroup of 8 waves per (b, s, f):
//                 p[t] = mean_m |S[m, t]|^2, w[t] = 1 / max(p[t], power_floor max_t p[t])  (a first sweep over S for the maximum);
//                 the weighted Gram matrix of the stacked vector by the scheme of stacked_gram.hpp, which wpe_bin_k shares
//                 -- hence the stacking order s = [z; y] INSIDE the kernel (the interface order is [y; z]) -- and beside it,
//                 on the last wave, the unweighted Gram tile of [Re S; Im S] (2 M <= 16 rows: one tile), which gives
//                 Phi_s = S S^H / T;
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
#include "stacked_gram.hpp"

namespace mn {

constexpr int WPD_LDS_LIMIT = 160 * 1024;

// workspace: fail int [B S F] | wbar c128 [B S F][K] (interface order [y; z])
struct WpdWs { long long fail, w, total; };
__host__ __device__ inline WpdWs wpd_ws(int B, int S, int F, int M, int taps) {
  WpdWs w;
  const long long bins = (long long)B * S * F;
  w.fail = 0;
  w.w = sg_align(bins * 4);
  w.total = sg_align(w.w + bins * M * (taps + 1) * 16);
  return w;
}
long long wpd_ws_bytes(int B, int S, int F, int M, int taps) { return wpd_ws(B, S, F, M, taps).total; }

// LDS of wpd_bin_k, in bytes from the start of the dynamic block
struct WpdLds { int R, col, X, wb, wt, red, part, zwin, ywin, swin, zero, total, zp; };
__host__ __device__ inline WpdLds wpd_lds(int M, int taps) {
  const int N = M * taps, K = N + M;
  WpdLds l;
  l.zp = sg_zpitch(taps);
  l.R = 0;                                                             // double2 [K][K], lower triangle
  l.col = l.R + K * K * 16;                                            // double2 [K]
  l.X = l.col + K * 16;                                                // double2 [M][K]: the right-hand sides, one per row
  l.wb = l.X + M * K * 16;                                             // double2 [K]: wbar in the kernel's order [z; y]
  l.wt = l.wb + K * 16;                                                // double [TT]
  l.red = l.wt + SG_TT * 8;                                            // double [WAVES]
  l.part = l.red + SG_WAVES * 8;                                       // double2 [WAVES][TT] of the apply; before it double [16][16]
  l.zwin = l.part + SG_WAVES * SG_TT * 16;                             // float [2 M][zp]: frames t0 - delay - (taps - 1) ...
  l.ywin = l.zwin + 2 * M * l.zp * 4;                                  // float [2 M][TT]: frames t0 ...
  l.swin = l.ywin + 2 * M * SG_TT * 4;                                 // float [2 M][TT]: the source estimate
  l.zero = l.swin + 2 * M * SG_TT * 4;                                 // float [TT] of zeros: the rows past 2 K / 2 M
  l.total = l.zero + SG_TT * 4;
  return l;
}
int wpd_lds_bytes(int M, int taps) { return wpd_lds(M, taps).total; }

// grid (F, B, S), 512 threads, wpd_lds(M, taps).total bytes of dynamic LDS
__global__ __launch_bounds__(SG_THREADS) void wpd_bin_k(const WpdArgs a, const COut out, int* fail_out, double2* w_out) {
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
  const SgWin win = {l.zwin, l.ywin, l.zero, zp};
  // the observation and the source estimate of this bin, as launch_mvdr reads them
  const long long yoff = (long long)b * a.mix.sb + (long long)f * a.mix.sf;
  const float* yre = a.mix.re + yoff;
  const float* yim = a.mix.im + yoff;
  const long long yst = a.mix.st;
  const auto load_y = [&](int m, int t) {
    return make_float2(yre[(long long)m * a.mix.sm + t * yst], yim[(long long)m * a.mix.sm + t * yst]);
  };
  const auto load_s = [&](int m, int t) {
    const float *sre, *sim;
    int sst;
    src_row(a, b, f, m, spk, sre, sim, sst);
    return make_float2(sre[(long long)t * sst], sim[(long long)t * sst]);
  };
  const int ntile_t = (T + SG_TT - 1) / SG_TT;
  const long long oo = (long long)b * out.ob + (long long)spk * out.os + (long long)f * out.of;
  float* ore = out.re + oo;
  float* oim = out.im + oo;

  if (tid < SG_TT) zero[tid] = 0.f;

  // ---- the maximum of p[t] = mean_m |S[m, t]|^2 (the same arithmetic as below, on the same float32 values)
  double pm = 0.0;
  for (int t = tid; t < T; t += SG_THREADS) {
    double p = 0.0;
    for (int m = 0; m < M; ++m) {                                      // fixed order: microphone 0, 1, ...
      const float2 v = load_s(m, t);
      const double xr = (double)v.x, xi = (double)v.y;
      p = fma(xr, xr, p);
      p = fma(xi, xi, p);
    }
    pm = fmax(pm, p / (double)M);
  }
  const double thr = a.power_floor * sg_block_max(pm, red);

  SgTiles g;
  sg_tiles_init(g, M, N, K, taps, win);
  // the one tile of [Re S; Im S]: row lr of it, both operands (the last wave has the fewest tiles of the other kind)
  const int offS = (lr < 2 * M ? (l.swin - l.zwin) / 4 + lr * SG_TT : (l.zero - l.zwin) / 4) + lg;
  const bool src_wave = wave == SG_WAVES - 1;                          // wave-uniform

  // ---- the Gram matrix of [Re s; Im s], w folded into B; the Gram tile of the source estimate
  sg_gram_zero(g);
  d4 accs = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * SG_TT;
    __syncthreads();
    sg_stage(load_y, M, T, taps, a.delay, t0, true, zwin, ywin, zp);
    sg_stage_rows(load_s, M, T, t0, swin);
    __syncthreads();
    if (tid < SG_TT) {
      double p = 0.0;
      for (int m = 0; m < M; ++m) {
        const double xr = (double)swin[m * SG_TT + tid], xi = (double)swin[(M + m) * SG_TT + tid];
        p = fma(xr, xr, p);
        p = fma(xi, xi, p);
      }
      wt[tid] = t0 + tid < T ? 1.0 / fmax(p / (double)M, thr) : 0.0;
    }
    __syncthreads();
    sg_gram_tile(g, zwin, wt, [&](int k4) {
      if (src_wave) {
        const double sv = (double)zwin[offS + k4];
        accs = __builtin_amdgcn_mfma_f64_16x16x4f64(sv, sv, accs, 0, 0, 0);
      }
    });
  }

  // ---- R (lower triangle) from the blocks of the Gram matrix; the Gram tile of the source beside it
  sg_panel(g, K, K, R);
  if (src_wave) {
#pragma unroll
    for (int r = 0; r < 4; ++r) gs[(lg + 4 * r) * 16 + lr] = accs[r];
  }
  __syncthreads();
  // Phibar as the right-hand sides: X[c][N + i] = Phi_s[i][c] = (S S^H)[i][c] / T from its lower triangle (Hermitian by
  // construction, a real diagonal); rows < N are 0.  Re = G[i][j] + G[M + i][M + j], Im = G[M + i][j] - G[M + j][i]
  for (int e = tid; e < M * K; e += SG_THREADS) {
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
  if (a.diag_load != 0.0) sg_diag_load(R, K, a.diag_load, red);
  __syncthreads();

  bool failed = !sg_cholesky(R, K, K, col);

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
      for (int e = tid; e < M * i; e += SG_THREADS) {
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
      for (int r = tid; r < K; r += SG_THREADS) {
        const double2 v = X[a.ref * K + r];
        const double2 w = make_double2((v.x * tr_re + v.y * tr_im) / den, (v.y * tr_re - v.x * tr_im) / den);
        wb[r] = w;
        wg[r >= N ? r - N : M + r] = w;                                // interface order [y; z]
      }
    }
  }

  if (failed) {                                                        // uniform
    if (tid == 0) fail_out[bin] = 1;
    for (int r = tid; r < K; r += SG_THREADS) wg[r] = make_double2(0.0, 0.0);
    for (int t = tid; t < T; t += SG_THREADS) {
      ore[(long long)t * out.ot] = 0.f;
      oim[(long long)t * out.ot] = 0.f;
    }
    return;
  }
  if (tid == 0) fail_out[bin] = 0;

  // ---- out[t] = wbar^H s[t]: wave v adds the rows v, v + 8, ... of a frame, the eight partial sums are added in wave order
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * SG_TT;
    __syncthreads();
    sg_stage(load_y, M, T, taps, a.delay, t0, true, zwin, ywin, zp);
    __syncthreads();
    double sr = 0.0, si = 0.0;
    for (int r = wave; r < K; r += SG_WAVES) {
      const double2 w = wb[r];
      double vr, vi;
      if (r < N) {
        const int k = r / M, m = r - k * M, zo = lane + taps - 1 - k;
        vr = (double)zwin[m * zp + zo];
        vi = (double)zwin[(M + m) * zp + zo];
      } else {
        vr = (double)ywin[(r - N) * SG_TT + lane];
        vi = (double)ywin[(M + r - N) * SG_TT + lane];
      }
      sr += w.x * vr + w.y * vi;                                       // conj(w) s
      si += w.x * vi - w.y * vr;
    }
    part[wave * SG_TT + lane] = make_double2(sr, si);
    __syncthreads();
    if (tid < SG_TT && t0 + tid < T) {
      double2 v = part[tid];
#pragma unroll
      for (int k = 1; k < SG_WAVES; ++k) { v.x += part[k * SG_TT + tid].x; v.y += part[k * SG_TT + tid].y; }
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
  hipLaunchKernelGGL(wpd_bin_k, dim3(a.F, a.B, a.S), dim3(SG_THREADS), lds, s, a, out, reinterpret_cast<int*>(base + w.fail),
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
