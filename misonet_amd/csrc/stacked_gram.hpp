// The stacked-Gram bin solver shared by wpe_bin_k (wpe.hip) and wpd_bin_k (wpd.hip): every piece of the two kernels that is the
// same float64 code lives here, once.
//
// One workgroup of 8 waves owns a bin.  With N = M taps and the stacked vector s[t] = [z[t]; y[t]] of order K = N + M,
// z[(k M + m), t] = y[m, t - delay - k], the scheme is
//
//   sg_stage        T is tiled through LDS, SG_TT frames at a time: a z window (taps - 1 frames of history in front, odd row
//                   pitch) and a y window, real parts in rows [0, M), imaginary parts in rows [M, 2 M), float32 as read
//   sg_gram_tile    the real Gram matrix of [Re s; Im s] (2 K rows, 16 x 16 tiles, lower half) on v_mfma_f64_16x16x4_f64 with
//                   the weight w[t] folded into the B operand; the tiles are dealt round-robin to the waves (SgTiles), up to
//                   SG_SLOTS accumulators each, which reaches 2 K = 176
//   sg_gram_tile1   the one-tile case (2 n <= 16 float64 rows staged frame-major, one wave; cacgmm_bin_k of cacgmm.hip, which also
//                   uses sg_stage_rows, sg_diag_load and sg_cholesky) and sg_tile1_entry, the complex entry from such a tile
//   sg_panel        its blocks give the complex panel sum_t w s s^H, lower triangle, the first `ncols` columns, in four
//                   phases in which every component is written by one lane
//   sg_diag_load    + diag_load tr / n on the leading n x n block
//   sg_cholesky     column by column in LDS on a rows x ncols panel; rows below the square block leave it as the solution
//                   of the forward substitution
//
// Every sum runs in a fixed order and nothing is accumulated with atomics: the callers' results are bit-reproducible.  A
// pivot that is not finite or not > 0 (the all-zero bin: w infinite, the panel NaN) ends the factorisation; what follows is
// the caller's.  Every helper is called by all SG_THREADS threads of the workgroup.
#pragma once
#include <hip/hip_runtime.h>

namespace mn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int SG_TT = 64;             // frames per LDS tile: 75 KB of LDS at M = 6, 10 taps in WPE -- two workgroups per CU
constexpr int SG_THREADS = 512;       // 8 waves
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int SG_SLOTS = 9;           // 16 x 16 tiles per wave: ceil(66 / 8) at the largest 2 K = 176

__host__ __device__ inline long long sg_align(long long x) { return (x + 255) & ~255LL; }
// row pitch of the z window, in floats (odd)
__host__ __device__ inline int sg_zpitch(int taps) { return (SG_TT + taps - 1) | 1; }

// the staged windows of a kernel, in bytes from the start of its dynamic LDS block (zero: SG_TT floats of zeros, the rows past
// 2 K), and the row pitch of the z window
struct SgWin { int zwin, ywin, zero, zp; };

// where row rho of [Re s; Im s] starts in the staged windows (float index from zwin), so that + tl gives frame t0 + tl
__device__ __forceinline__ int sg_row_off(int rho, int M, int N, int K, int taps, const SgWin& l) {
  if (rho >= 2 * K) return (l.zero - l.zwin) / 4;
  const int part = rho >= K ? 1 : 0, q = rho - part * K;
  if (q < N) {
    const int k = q / M, m = q - k * M;
    return (part * M + m) * l.zp + (taps - 1 - k);
  }
  return (l.ywin - l.zwin) / 4 + (part * M + (q - N)) * SG_TT;
}

// tile number tau, counted row by row over the lower half, -> (I, J); an unused slot reads as tile 0
__device__ __forceinline__ void sg_tile(int tau, int ntiles, int& I, int& J) {
  if (tau >= ntiles) tau = 0;
  I = 0;
  while (tau > I) { tau -= I + 1; ++I; }
  J = tau;
}

// stages frames t0 ... of the M rows load(m, t) -> float2 into win [2 M][SG_TT]: real parts in rows [0, M), imaginary in [M, 2 M)
template <typename Load>
__device__ __forceinline__ void sg_stage_rows(Load load, int M, int T, int t0, float* win) {
  for (int e = threadIdx.x; e < M * SG_TT; e += SG_THREADS) {
    const int m = e / SG_TT, i = e - m * SG_TT, t = t0 + i;
    float2 v = {0.f, 0.f};
    if (t < T) v = load(m, t);
    win[m * SG_TT + i] = v.x;
    win[(M + m) * SG_TT + i] = v.y;
  }
}

// stages the frames of tile t0: the z window (when asked) and the y window
template <typename Load>
__device__ __forceinline__ void sg_stage(Load load, int M, int T, int taps, int delay, int t0, bool want_z, float* zwin,
                                         float* ywin, int zp) {
  if (want_z) {
    const int zl = SG_TT + taps - 1, tb = t0 - delay - (taps - 1);
    for (int e = threadIdx.x; e < M * zl; e += SG_THREADS) {
      const int m = e / zl, i = e - m * zl, t = tb + i;
      float2 v = {0.f, 0.f};
      if (t >= 0 && t < T) v = load(m, t);
      zwin[m * zp + i] = v.x;
      zwin[(M + m) * zp + i] = v.y;
    }
  }
  sg_stage_rows(load, M, T, t0, ywin);
}

// the maximum of pm over the workgroup, the same value on every thread; red: double [SG_WAVES].  Holds one barrier
__device__ __forceinline__ double sg_block_max(double pm, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) pm = fmax(pm, __shfl_xor(pm, k, 64));
  if (lane == 0) red[wave] = pm;
  __syncthreads();
  pm = red[0];
#pragma unroll
  for (int k = 1; k < SG_WAVES; ++k) pm = fmax(pm, red[k]);
  return pm;
}

// the 16 x 16 tiles (I >= J) of the 2 K x 2 K Gram matrix a wave owns: tile number wave + 8 slot, counted row by row; offA /
// offB: this lane's operand rows in the windows (float index from zwin), acc: the accumulators
struct SgTiles {
  int offA[SG_SLOTS], offB[SG_SLOTS];
  int ntiles, nslots;                                                  // nslots: wave-uniform
  d4 acc[SG_SLOTS];
};

__device__ __forceinline__ void sg_tiles_init(SgTiles& g, int M, int N, int K, int taps, const SgWin& l) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const int NT = (2 * K + 15) / 16;
  g.ntiles = NT * (NT + 1) / 2;
#pragma unroll
  for (int s = 0; s < SG_SLOTS; ++s) {
    int I, J;
    sg_tile(wave + SG_WAVES * s, g.ntiles, I, J);
    g.offA[s] = sg_row_off(16 * I + lr, M, N, K, taps, l) + lg;        // A[i = lr][k = lg], B[k = lg][j = lr]
    g.offB[s] = sg_row_off(16 * J + lr, M, N, K, taps, l) + lg;
  }
  g.nslots = __builtin_amdgcn_readfirstlane(wave < g.ntiles ? (g.ntiles - 1 - wave) / SG_WAVES + 1 : 0);
}

__device__ __forceinline__ void sg_gram_zero(SgTiles& g) {
#pragma unroll
  for (int s = 0; s < SG_SLOTS; ++s) g.acc[s] = d4{0.0, 0.0, 0.0, 0.0};
}

// adds the staged tile to the Gram matrix: acc += A (B w) over its SG_TT frames, wt: double [SG_TT] (0 past T).  extra(k4) runs
// between the loads of a step and its MFMAs
template <typename Extra>
__device__ __forceinline__ void sg_gram_tile(SgTiles& g, const float* zwin, const double* wt, Extra extra) {
  const int lg = (threadIdx.x & 63) >> 4;
#pragma unroll 1
  for (int k4 = 0; k4 < SG_TT; k4 += 4) {                              // the loads of a step first, then its MFMAs
    const double wv = wt[k4 + lg];
    float av[SG_SLOTS], bv[SG_SLOTS];
#pragma unroll
    for (int s = 0; s < SG_SLOTS; ++s)
      if (s < g.nslots) {                                              // wave-uniform
        av[s] = zwin[g.offA[s] + k4];
        bv[s] = zwin[g.offB[s] + k4];
      }
    extra(k4);
#pragma unroll
    for (int s = 0; s < SG_SLOTS; ++s)
      if (s < g.nslots)
        g.acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[s], (double)bv[s] * wv, g.acc[s], 0, 0, 0);
  }
}

// The one-tile case (2 n <= 16 rows, cacgmm_bin_k): rows = [Re v; Im v] as float64, staged frame-major, double [SG_TT][pitch]
// with the rows past 2 n zero.  acc += sum_t w[t] r[t] r[t]^T over the SG_TT frames of the tile, in ascending t; called by one
// whole wave
__device__ __forceinline__ void sg_gram_tile1(d4& acc, const double* rows, int pitch, const double* wt) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
#pragma unroll 4
  for (int k4 = 0; k4 < SG_TT; k4 += 4) {
    const double v = rows[(k4 + lg) * pitch + lr];                     // A[i = lr][k = lg], B[k = lg][j = lr]
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v * wt[k4 + lg], acc, 0, 0, 0);
  }
}

// element (i, j), i >= j, of the complex n x n matrix sum w v v^H from that tile, g: double [16][16] as the accumulator left it
// (row = (lane >> 4) + 4 reg, column = lane & 15): Re = G[i][j] + G[n + i][n + j], Im = G[n + i][j] - G[n + j][i], a real
// diagonal
__device__ __forceinline__ double2 sg_tile1_entry(const double* g, int n, int i, int j) {
  return make_double2(g[i * 16 + j] + g[(n + i) * 16 + n + j], i == j ? 0.0 : g[(n + i) * 16 + j] - g[(n + j) * 16 + i]);
}

// the complex panel P [K][ncols] (lower triangle of its square block; ncols < K: the rows below it too) from the blocks of
// the Gram matrix.  Element (rho_i, rho_j), rho = part K + q:
//   phase 0  Re Re:  P[qi][qj].re  = g        phase 2  Im Re, qi >= qj:  P[qi][qj].im  = g
//   phase 1  Im Im:  P[qi][qj].re += g        phase 3  Im Re, qi <= qj:  P[qj][qi].im -= g
// every component is written by one lane per phase; C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg.  A
// barrier stands in front of every phase, none behind the last
__device__ __forceinline__ void sg_panel(const SgTiles& g, int K, int ncols, double2* P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane & 15, lg = lane >> 4;
#pragma unroll 1
  for (int ph = 0; ph < 4; ++ph) {
    __syncthreads();
#pragma unroll
    for (int s = 0; s < SG_SLOTS; ++s)
      if (s < g.nslots) {
        int I, J;
        sg_tile(wave + SG_WAVES * s, g.ntiles, I, J);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ri = 16 * I + lg + 4 * r, rj = 16 * J + lr;
          if (ri < rj || ri >= 2 * K) continue;
          const int pi = ri >= K, pj = rj >= K, qi = ri - pi * K, qj = rj - pj * K;
          const double v = g.acc[s][r];
          if (ph == 0 && !pi && !pj && qj < ncols) P[qi * ncols + qj].x = v;
          if (ph == 1 && pi && pj && qj < ncols) P[qi * ncols + qj].x += v;
          if (ph == 2 && pi && !pj && qi >= qj && qj < ncols) P[qi * ncols + qj].y = v;
          if (ph == 3 && pi && !pj && qi <= qj && qi < ncols) P[qj * ncols + qi].y -= v;
        }
      }
  }
}

// P[i][i] += load tr / n over the leading n x n block of P (pitch n), the trace added in index order by one thread; red: one
// double.  Starts behind a barrier and ends without one
__device__ __forceinline__ void sg_diag_load(double2* P, int n, double load, double* red) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    double tr = 0.0;
    for (int i = 0; i < n; ++i) tr += P[i * n + i].x;
    red[0] = load * tr / (double)n;
  }
  __syncthreads();
  if (tid < n) P[tid * n + tid].x += red[0];
}

// Cholesky of the panel P [rows][ncols], column by column, three barriers per column; col: double2 [rows].  Every thread sees
// the same pivot: false (on every thread, at once) at one that is not finite or not > 0
__device__ __forceinline__ bool sg_cholesky(double2* P, int rows, int ncols, double2* col) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
  for (int c = 0; c < ncols; ++c) {
    const double piv = P[c * ncols + c].x;
    if (!(piv > 0.0) || !(piv <= 1.7976931348623157e308)) return false;
    const double d = sqrt(piv);
    __syncthreads();                                                   // the pivot is read before the column is rewritten
    for (int i = c + tid; i < rows; i += SG_THREADS) {
      double2 v = P[i * ncols + c];
      if (i == c) v = make_double2(d, 0.0);
      else { v.x /= d; v.y /= d; }
      col[i] = v;
      P[i * ncols + c] = v;
    }
    __syncthreads();
    for (int j = c + 1 + tx; j < ncols; j += 16) {
      const double2 lj = col[j];
      for (int i = c + 1 + ty; i < rows; i += SG_THREADS / 16)
        if (i >= j) {
          const double2 li = col[i];
          double2 v = P[i * ncols + j];
          v.x -= li.x * lj.x + li.y * lj.y;                            // l_i conj(l_j)
          v.y -= li.y * lj.x - li.x * lj.y;
          P[i * ncols + j] = v;
        }
    }
    __syncthreads();
  }
  return true;
}

}  // namespace mn
