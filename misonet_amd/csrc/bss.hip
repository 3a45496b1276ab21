// BSS-eval (Vincent et al. 2006) on the device: the energies behind SDR, SIR and SAR (C ABI misonet_bss_corr / misonet_bss_solve
// in net.hip; the definitions are restated in NumPy in tests/bss_ref.py, the dB figures are formed on the host in score.py).
//
//   bss_corr_k       part[item][segment][pair][lag] = sum over the 4096 products of one segment of x[t] y[t + lag], on the
//                    float64 matrix pipe: with A[v][k] = x[t0 + k - v] and B[k][u] = y[t0 + k + 16 u] the 16 x 16 product
//                    collects lag 16 u + v, so one v_mfma_f64_16x16x4_f64 chain yields 256 lags
//   bss_corr_fold_k  Rrr / Rre / Eee = the segments added in segment order (an int16 estimate scaled once, after the sums)
//   bss_assemble_k   per item 1 + R dense systems, lower triangle, with the right-hand sides as E extra ROWS below the matrix:
//                    system 0 = G (order R Q, block Toeplitz) over D, system 1 + j = G_jj (order Q) over d_.j
//   bss_panel_k      one 64-column panel: every workgroup factors the 64 x 64 diagonal block in LDS (redundantly: the same
//                    code on the same numbers, so the same bits) and solves one row per thread against it.  The extra rows
//                    ride along: when the last panel is done they hold (L^-1 D)^T -- the forward substitution is free
//   bss_update_k     trailing update C -= P_i P_j^T of the lower 64 x 64 tiles on the float64 MFMA
//   bss_finish_k     T / A = the squared norm of an extra row, added in a fixed order; NaN where the factorisation failed
//
// Every sum runs in a fixed order, nothing is accumulated with atomics and a system never looks at another one: the result
// of an item is bit-reproducible and does not depend on the batch it sits in or on its position there.
#include "kernels.hpp"

namespace mn {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int BSS_SEG = 4096;         // k values per workgroup of bss_corr_k (as score_wave_k)
constexpr int BSS_CH = 1024;          // k values staged in LDS at a time
constexpr int BSS_TILE = 256;         // lags per wave: one 16 x 16 accumulator
constexpr int BSS_YS = BSS_CH + 1024; // y window of a staging round: BSS_CH + the largest Q
constexpr int BSS_NB = 64;            // panel width of the factorisation (DESIGN: 32 KB diagonal block + 64 row values per thread)
constexpr int BSS_XROWS = 4;          // rows reserved below every system for the right-hand sides (E <= 4)

// sample m of the signal at `base` of a view as stored (an int16 estimate is scaled after the sums), zero outside [0, nv)
__device__ __forceinline__ float bss_ld(const SigView& v, long long base, long long m, long long nv) {
  return m < 0 || m >= nv ? 0.0f : sig_raw(v, base, m);
}

__device__ __forceinline__ int bss_ypos(int i) { return i + (i >> 4); }   // one pad word per 16: the stride-16 reads of B spread over the banks

// grid (segments, pairs, items), 64 * ceil(Q / 256) threads: wave w owns lags [256 w, 256 w + 256).
// pair p < R R: (r_j, r_k), j = p / R; p < R R + R E: (r_j, e_i), j = q / E; else (e_i, e_i), of which only lag 0 is kept.
// Segment s covers k in [4096 s, 4096 s + 4096) where row v of A reads x[k - v]: ceil((n + 15) / 4096) segments reach every
// product.  Two accumulator chains (even and odd steps) are added once at the end.
__global__ __launch_bounds__(256) void bss_corr_k(const SigView ve, const SigView vr, int E, int R, int Q, long long n,
                                                  const int* n_valid, double* part) {
  __shared__ float xs[BSS_CH + 16];
  __shared__ float ys[BSS_YS + BSS_YS / 16 + 1];
  const int seg = blockIdx.x, p = blockIdx.y, b = blockIdx.z;
  const int NP = R * R + R * E + E;
  const long long nv = sig_nv(n_valid, b, n);
  const long long be = (long long)b * ve.sb, br = (long long)b * vr.sb;
  SigView x = vr, y = vr;
  long long xo, yo;
  int tiles = (Q + BSS_TILE - 1) / BSS_TILE;
  if (p < R * R) {
    xo = br + (long long)(p / R) * vr.ss;
    yo = br + (long long)(p % R) * vr.ss;
  } else if (p < R * R + R * E) {
    const int q = p - R * R;
    xo = br + (long long)(q / E) * vr.ss;
    y = ve;
    yo = be + (long long)(q % E) * ve.ss;
  } else {
    x = y = ve;
    xo = yo = be + (long long)(p - R * R - R * E) * ve.ss;
    tiles = 1;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int v = lane & 15, g = lane >> 4;                              // v: row of A and column of B of this lane; g: its k
  const bool active = wave < tiles;
  const int ywin = BSS_CH + tiles * BSS_TILE;
  d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  const long long k_seg = (long long)seg * BSS_SEG;
#pragma unroll 1
  for (int c = 0; c < BSS_SEG / BSS_CH; ++c) {
    const long long k0 = k_seg + (long long)c * BSS_CH;
    if (k0 - 15 >= nv) break;                                          // x is zero from here on: the sums do not move
    __syncthreads();
    for (int i = threadIdx.x; i < BSS_CH + 15; i += blockDim.x) xs[i] = bss_ld(x, xo, k0 - 15 + i, nv);
    for (int i = threadIdx.x; i < ywin; i += blockDim.x) ys[bss_ypos(i)] = bss_ld(y, yo, k0 + i, nv);
    __syncthreads();
    if (active) {
      const int xb = g - v + 15, yb = g + wave * BSS_TILE + 16 * v;    // A[v][g] = x[k - v], B[g][u = v] = y[k + 16 u] at k = k0 + 4 s + g
#pragma unroll 4
      for (int s = 0; s < BSS_CH / 4; s += 2) {
        const double a0 = (double)xs[xb + 4 * s], b0 = (double)ys[bss_ypos(yb + 4 * s)];
        const double a1 = (double)xs[xb + 4 * s + 4], b1 = (double)ys[bss_ypos(yb + 4 * s + 4)];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc1, 0, 0, 0);
      }
    }
  }
  if (active) {
    // C/D of the f64 MFMA: column = lane & 15 (u), row = (lane >> 4) + 4 reg (v)
    double* q = part + (((long long)b * gridDim.x + seg) * NP + p) * Q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lag = wave * BSS_TILE + 16 * v + g + 4 * r;
      if (lag < Q) q[lag] = acc0[r] + acc1[r];
    }
  }
}

// grid (pairs, items), 256 threads over the lags
__global__ __launch_bounds__(256) void bss_corr_fold_k(const double* part, int nseg, int E, int R, int Q, double ce,
                                                       double* Rrr, double* Rre, double* Eee) {
  const int p = blockIdx.x, b = blockIdx.y;
  const int NP = R * R + R * E + E;
  const bool ee = p >= R * R + R * E;
  const int na = ee ? 1 : Q;
  for (int a = threadIdx.x; a < na; a += 256) {
    const double* q = part + ((long long)b * nseg * NP + p) * Q + a;
    double s = 0.0;
    for (int k = 0; k < nseg; ++k) s += q[(long long)k * NP * Q];      // fixed order: segment 0, 1, ...
    if (p < R * R) Rrr[((long long)b * R * R + p) * Q + a] = s;
    else if (!ee) Rre[((long long)b * R * E + (p - R * R)) * Q + a] = s * ce;
    else Eee[(long long)b * E + (p - R * R - R * E)] = s * (ce * ce);
  }
}

long long bss_corr_segments(long long n) { return (n + 15 + BSS_SEG - 1) / BSS_SEG; }

hipError_t launch_bss_corr(const SigView& est, const SigView& ref, int B, int E, int R, long long n, const int* n_valid, int Q,
                           double* part, double* Rrr, double* Rre, double* Eee, hipStream_t s) {
  const int nseg = (int)bss_corr_segments(n), NP = R * R + R * E + E;
  const int tiles = (Q + BSS_TILE - 1) / BSS_TILE;
  hipLaunchKernelGGL(bss_corr_k, dim3(nseg, NP, B), dim3(64 * tiles), 0, s, est, ref, E, R, Q, n, n_valid, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(bss_corr_fold_k, dim3(NP, B), dim3(256), 0, s, part, nseg, E, R, Q, sig_unit(est), Rrr, Rre, Eee);
  return hipGetLastError();
}

// ---- the systems ------------------------------------------------------------------------------------------------------
// Item b owns bss_item_doubles(R, Q) doubles of scratch: system 0 (order N = R Q, N + 4 rows of N) and then the R systems of
// order Q (Q + 4 rows of Q each), all row-major with the row length = the order.
__host__ __device__ inline long long bss_item_doubles(int R, int Q) {
  const long long N = (long long)R * Q;
  return (N + BSS_XROWS) * N + (long long)R * (Q + BSS_XROWS) * Q;
}
struct BssSys { double* m; int n; int j; };                            // j = -1: the full system; else the reference of G_jj
__device__ __forceinline__ BssSys bss_sys(double* scratch, int b, int sys, int R, int Q) {
  double* base = scratch + (long long)b * bss_item_doubles(R, Q);
  const long long N = (long long)R * Q;
  if (sys == 0) return {base, (int)N, -1};
  return {base + (N + BSS_XROWS) * N + (long long)(sys - 1) * (Q + BSS_XROWS) * Q, Q, sys - 1};
}
__device__ __forceinline__ bool bss_silent(const double* Rrr, int b, int R, int Q, int j) {
  return Rrr[(((long long)b * R + j) * R + j) * Q] == 0.0;
}

// grid (R Q + E rows, 1 + R systems, items), 256 threads over the columns up to the diagonal
__global__ __launch_bounds__(256) void bss_assemble_k(const double* Rrr, const double* Rre, int E, int R, int Q, double* scratch,
                                                      int* info) {
  const int row = blockIdx.x, sys = blockIdx.y, b = blockIdx.z;
  if (row == 0 && sys == 0 && threadIdx.x == 0) info[b] = -1;
  const BssSys S = bss_sys(scratch, b, sys, R, Q);
  if (row >= S.n + E) return;
  const double* rr = Rrr + (long long)b * R * R * Q;
  const double* re = Rre + (long long)b * R * E * Q;
  double* out = S.m + (long long)row * S.n;
  if (row >= S.n) {                                                    // right-hand side i as a row: D_i^T
    const int i = row - S.n;
    for (int col = threadIdx.x; col < S.n; col += 256) {
      const int k = S.j < 0 ? col / Q : S.j, c = S.j < 0 ? col % Q : col;
      out[col] = bss_silent(Rrr, b, R, Q, k) ? 0.0 : re[((long long)k * E + i) * Q + c];
    }
    return;
  }
  const int j = S.j < 0 ? row / Q : S.j, a = S.j < 0 ? row % Q : row;
  const bool sj = bss_silent(Rrr, b, R, Q, j);
  for (int col = threadIdx.x; col <= row; col += 256) {
    const int k = S.j < 0 ? col / Q : S.j, c = S.j < 0 ? col % Q : col;
    double v;
    if (sj || bss_silent(Rrr, b, R, Q, k)) v = col == row ? 1.0 : 0.0;  // a silent reference leaves the span
    else v = a >= c ? rr[((long long)j * R + k) * Q + (a - c)] : rr[((long long)k * R + j) * Q + (c - a)];
    out[col] = v;
  }
}

// grid (row blocks, 1 + R systems, items), 256 threads; panel = columns [pc, pc + 64) of every system that has them.
// Workgroup x solves rows pc + 64 + 256 x + thread (pc + w + ... behind a narrower last panel).  The diagonal block is never written back: nothing reads it again.
__global__ __launch_bounds__(256) void bss_panel_k(const double* Rrr, int E, int R, int Q, int pc, double* scratch, int* info) {
  __shared__ double Ls[BSS_NB][BSS_NB + 1];
  __shared__ double col[BSS_NB];
  const int sys = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const BssSys S = bss_sys(scratch, b, sys, R, Q);
  if (pc >= S.n) return;
  const int w = S.n - pc < BSS_NB ? S.n - pc : BSS_NB;
  const int row = pc + w + blockIdx.x * 256 + tid;                     // w < 64 only in a system's last panel: the extra rows follow
  if (pc + w + (int)blockIdx.x * 256 >= S.n + E && blockIdx.x != 0) return;
  // the diagonal block, lower triangle; the identity where the panel is narrower than 64
  for (int e = tid; e < BSS_NB * BSS_NB; e += 256) {
    const int i = e / BSS_NB, j = e % BSS_NB;
    double v = 0.0;
    if (j <= i) v = i < w ? S.m[(long long)(pc + i) * S.n + pc + j] : (i == j ? 1.0 : 0.0);
    Ls[i][j] = v;
  }
  int bad = -1;
  for (int c = 0; c < BSS_NB; ++c) {
    __syncthreads();
    const double piv = Ls[c][c];
    if (tid == 0 && bad < 0 && c < w) {
      // the pivot against 2^-40 of the matching diagonal entry of G (1 for a silent reference's identity block)
      const int j = S.j < 0 ? (pc + c) / Q : S.j;
      double gd = Rrr[(((long long)b * R + j) * R + j) * Q];
      if (gd == 0.0) gd = 1.0;
      if (!(piv > gd * 0x1p-40) || !(fabs(piv) <= 1.7976931348623157e308)) bad = pc + c;
    }
    const double d = sqrt(piv);
    if (tid < BSS_NB) col[tid] = tid > c ? Ls[tid][c] / d : (tid == c ? d : 0.0);
    __syncthreads();
    for (int e = tid; e < BSS_NB * BSS_NB; e += 256) {
      const int i = e / BSS_NB, j = e % BSS_NB;
      if (j > c && i >= j) Ls[i][j] -= col[i] * col[j];
      else if (j == c && i >= c) Ls[i][c] = col[i];
    }
  }
  __syncthreads();
  if (bad >= 0 && sys == 0 && blockIdx.x == 0 && info[b] < 0) info[b] = bad;   // thread 0 only; kernels run in panel order
  if (row >= S.n + E) return;
  // x L^T = a for one row, 16 columns at a time in registers: the solved columns to the left are read back from the row
  // itself (this thread wrote them), L is broadcast from LDS
  double* pr = S.m + (long long)row * S.n + pc;
#pragma unroll 1
  for (int cb = 0; cb < BSS_NB; cb += 16) {
    if (cb >= w) break;                                                // the order is a multiple of 16: whole groups only
    double x[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = pr[cb + c];
#pragma unroll 2
    for (int k = 0; k < cb; ++k) {
      const double xk = pr[k];
#pragma unroll
      for (int c = 0; c < 16; ++c) x[c] -= xk * Ls[cb + c][k];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) {
#pragma unroll
      for (int k = 0; k < c; ++k) x[c] -= x[k] * Ls[cb + c][cb + k];
      x[c] /= Ls[cb + c][cb + c];
    }
#pragma unroll
    for (int c = 0; c < 16; ++c) pr[cb + c] = x[c];
  }
}

// grid (row tiles, column tiles, (1 + R) items), 256 threads; tile (ib, jb) = (p + 1 + x, p + 1 + y) in units of 64, ib >= jb.
// Wave w owns rows 16 w .. 16 w + 15 of the tile and walks its four 16-column parts.  Lane (m, q) holds the 16 consecutive
// panel values k = 16 q .. 16 q + 15 of its row (128 contiguous bytes); step kk of the MFMA chain pairs k = 16 q + kk of both
// operands, so the chain of 16 steps covers the 64 columns of the panel.
__global__ __launch_bounds__(256) void bss_update_k(int E, int R, int Q, int pc, double* scratch) {
  const int sys = blockIdx.z % (1 + R), b = blockIdx.z / (1 + R);
  const BssSys S = bss_sys(scratch, b, sys, R, Q);
  const int p1 = pc / BSS_NB + 1;
  const int ib = p1 + blockIdx.x, jb = p1 + blockIdx.y;
  const int nrows = S.n + E;
  if (ib < jb || jb * BSS_NB >= S.n || ib * BSS_NB >= nrows) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, q = lane >> 4;
  const int i0 = ib * BSS_NB + wave * 16;
  if (i0 >= nrows) return;
  double a[16];
  {
    const int r = i0 + m;
    const double* src = S.m + (long long)r * S.n + pc + 16 * q;
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = r < nrows ? -src[k] : 0.0;
  }
#pragma unroll 1
  for (int t = 0; t < 4; ++t) {
    const int j0 = jb * BSS_NB + t * 16;
    if (j0 >= S.n) break;                                              // the order is a multiple of 16: whole parts only
    double bv[16];
    const double* src = S.m + (long long)(j0 + m) * S.n + pc + 16 * q;
#pragma unroll
    for (int k = 0; k < 16; ++k) bv[k] = src[k];
    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 reg
    d4 acc;
    double* c = S.m + (long long)(i0 + q) * S.n + j0 + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = i0 + q + 4 * r < nrows ? c[(long long)4 * r * S.n] : 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[k], bv[k], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i0 + q + 4 * r < nrows) c[(long long)4 * r * S.n] = acc[r];
  }
}

// grid (1 + R systems, items), 256 threads.  Thread t adds the squares of columns t, t + 256, ... in that order; 64-lane
// butterfly; the four waves in wave order.
__global__ __launch_bounds__(256) void bss_finish_k(int E, int R, int Q, const double* scratch, const int* info, double* T,
                                                    double* A) {
  __shared__ double s_tmp[4];
  const int sys = blockIdx.x, b = blockIdx.y;
  const BssSys S = bss_sys(const_cast<double*>(scratch), b, sys, R, Q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = 0; i < E; ++i) {
    const double* y = S.m + (long long)(S.n + i) * S.n;
    double v = 0.0;
    for (int c = threadIdx.x; c < S.n; c += 256) v += y[c] * y[c];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
    __syncthreads();
    if (lane == 0) s_tmp[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double r = (s_tmp[0] + s_tmp[1]) + (s_tmp[2] + s_tmp[3]);
      if (info[b] >= 0) r = __builtin_nan("");
      if (sys == 0) A[(long long)b * E + i] = r;
      else T[((long long)b * E + i) * R + (sys - 1)] = r;
    }
  }
}

long long bss_solve_doubles(int R, int Q) { return bss_item_doubles(R, Q); }

hipError_t launch_bss_solve(const double* Rrr, const double* Rre, int B, int E, int R, int Q, double* T, double* A, int* info,
                            double* scratch, hipStream_t s) {
  const int N = R * Q, nrows = N + E;
  hipLaunchKernelGGL(bss_assemble_k, dim3(nrows, 1 + R, B), dim3(256), 0, s, Rrr, Rre, E, R, Q, scratch, info);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  for (int pc = 0; pc < N; pc += BSS_NB) {
    const int below = nrows - pc - BSS_NB;                             // rows under the diagonal block (<= 0 in the last panel
    const int rb = below > 0 ? (below + 255) / 256 : 1;                //  of an order that is no multiple of 64: workgroup 0
    hipLaunchKernelGGL(bss_panel_k, dim3(rb, 1 + R, B), dim3(256), 0, s, Rrr, E, R, Q, pc, scratch, info);   // still tests the pivots)
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (pc + BSS_NB < N) {
      const int ti = (nrows - pc - BSS_NB + BSS_NB - 1) / BSS_NB, tj = (N - pc - BSS_NB + BSS_NB - 1) / BSS_NB;
      hipLaunchKernelGGL(bss_update_k, dim3(ti, tj, (1 + R) * B), dim3(256), 0, s, E, R, Q, pc, scratch);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  hipLaunchKernelGGL(bss_finish_k, dim3(1 + R, B), dim3(256), 0, s, E, R, Q, scratch, info, T, A);
  return hipGetLastError();
}

}  // namespace mn
