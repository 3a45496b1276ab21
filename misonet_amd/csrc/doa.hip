// Source localisation (include/misonet.h misonet_doa*): steered-response-power and MUSIC maps of a mixture
// over a table of candidate delays, and their peaks.  The project's own definition in the SRP-PHAT / MUSIC family (DiBiase 2000;
// Schmidt 1986); pyroomacoustics was not available and nothing here was compared against it.
//
//   mix complex64 [B, F, M, T], weight float32 [B, K, F, T] or none (K = 1, w = 1), tau float64 [Bg, D, M] seconds (Bg 1 or B),
//   pts float64 [D, 3];  nfft = 2 (F - 1) (2 when F = 1),  omega_f = 2 pi f fs / nfft;  float64 after the loads.
//   Blocks: block 0 = one block of T frames; hop 0 = block; N = 1 + (T - block) / hop; block n = frames [n hop, n hop + block).
//   1. per (b, k, n, f), f_lo <= f <= f_hi:  R = sum_t w[b,k,f,t] x~_t x~_t^H, t ascending over the block's frames; srp_phat:
//      x~_m = x_m / |x_m| (0 where x_m = 0), else x~ = x.  A bin with a non-finite sample, or a non-finite weight of class k, in
//      the block is skipped and fail |= 1; a bin with tr R = 0 is skipped.  srp, srp_phat: C_f = R.  music, S sources: the
//      eigenpairs of R by the beamformers' Jacobi, eigenvalues descending (equal ones: lower index first); lambda_{S-1} <=
//      1e-12 lambda_0: skipped; else C_f = (1 / M) sum_{r >= S} e_r e_r^H.  used = the bins not skipped; used = 0: fail |= 2, q = 0.
//   2. per (b, k, n, d):  q = g sum_{f used, ascending} ( sum_m C_f[m,m] + 2 Re sum_{m<n} C_f[m,n] e^{+j omega_f (tau_m - tau_n)} ),
//      g = 1 (srp kinds), 1 / used (music: q in [0, 1], small at a source).
//   3. per (b, k, n), S rounds: the best candidate left (max q; music: min q; ties: the lower index) is taken, then it and every
//      candidate with |pts_d - pts_best|^2 < min_sep^2 are retired.  peak -1 and value 0 once none is left.
//
// doa_cov_k (step 1): one wave per (b, n, f).  The block's frames are staged in chunks of DOA_FRAMES, normalised once for all K
// classes; lane (i, j), i <= j, owns element (i, j) of every class's R and adds its frames in ascending order; the lower triangle
// is the conjugate.  It writes C complex128 [B, K, N, F, M, M] and the per-bin state [B, K, N, F] (0 used, 1 non-finite, 2 skipped,
// 3 outside the band) into the workspace.
// doa_steer_k (step 2): one thread per candidate with its M delays in registers, the upper triangles of DOA_CHUNK bins staged in
// static LDS; z_m = e^{j omega tau_m} comes from float64 sincos at the first bin of every chunk and from a rotation by
// e^{j (omega_1 - omega_0) tau_m} for the bins behind it, and e^{j omega (tau_m - tau_n)} = z_m conj(z_n).
// doa_peak_k (step 3): one workgroup per (b, k, n); a candidate is retired when it lies within min_sep of an earlier peak, so no
// flags are kept.  It also counts used and raises fail.
// Every sum has one fixed order and every output has one writer: a recording's bits depend neither on B nor on its place.
#include "kernels.hpp"
#include "cplx.hpp"
#include "jacobi.hpp"

#include <cmath>

namespace mn {

constexpr int DOA_TILE = 256;            // candidates per workgroup of doa_steer_k; threads of doa_peak_k
constexpr int DOA_CHUNK = 16;            // bins per staged chunk of doa_steer_k
constexpr int DOA_FRAMES = 64;           // frames per staged chunk of doa_cov_k (= its threads)
constexpr double DOA_RANK_TOL = 1e-12;

int doa_tile() { return DOA_TILE; }
int doa_bin_chunk() { return DOA_CHUNK; }


// grid B N F (bin fastest), DOA_FRAMES threads
template <int M>
__global__ __launch_bounds__(DOA_FRAMES) void doa_cov_k(const float2* __restrict__ mix, const float* __restrict__ weight, int K,
                                                        int N, int F, int T, int block, int hop, int f_lo, int f_hi, int kind,
                                                        int S, double2* __restrict__ C, int* __restrict__ binst) {
  constexpr int MM = M * M;
  __shared__ double2 s_x[M][DOA_FRAMES];
  __shared__ double s_w[DOA_MAX_K][DOA_FRAMES];
  __shared__ double2 s_acc[DOA_MAX_K][MM];
  __shared__ double s_A[M][M][2], s_V[M][M][2];
  __shared__ int s_bad[1 + DOA_MAX_K];
  __shared__ int s_ord[M];
  const int tid = threadIdx.x;
  const long long id = blockIdx.x;
  const int f = (int)(id % F), n = (int)((id / F) % N), b = (int)(id / ((long long)F * N));
  const int i = tid / M, j = tid - i * M;
  const bool mine = tid < MM && i <= j;

  if (f < f_lo || f > f_hi) {                                        // block-uniform
    for (int k = 0; k < K; ++k) {
      const long long at = (((long long)b * K + k) * N + n) * F + f;
      if (tid < MM) C[at * MM + tid] = make_double2(0.0, 0.0);
      if (tid == 0) binst[at] = 3;
    }
    return;
  }

  if (tid < 1 + DOA_MAX_K) s_bad[tid] = 0;
  for (int k = 0; k < K; ++k)
    if (tid < MM) s_acc[k][tid] = make_double2(0.0, 0.0);
  const float2* x = mix + ((long long)b * F + f) * M * T;
  const int t0 = n * hop;
  for (int c0 = 0; c0 < block; c0 += DOA_FRAMES) {
    const int nt = block - c0 < DOA_FRAMES ? block - c0 : DOA_FRAMES;
    __syncthreads();
    const bool valid = tid < nt;
    const int t = t0 + c0 + (valid ? tid : 0);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float2 v = x[(long long)m * T + t];
      double re = (double)v.x, im = (double)v.y;
      if (valid && (!finite(v.x) || !finite(v.y))) s_bad[0] = 1;
      if (kind == DOA_SRP_PHAT) {
        const double a = sqrt(re * re + im * im);
        if (a > 0.0) { re /= a; im /= a; }
      }
      s_x[m][tid] = make_double2(re, im);
    }
    for (int k = 0; k < K; ++k) {
      float w = 1.0f;
      if (weight) w = weight[(((long long)b * K + k) * F + f) * T + t];
      if (valid && !finite(w)) s_bad[1 + k] = 1;
      s_w[k][tid] = (double)w;
    }
    __syncthreads();
    if (mine)
      for (int k = 0; k < K; ++k) {
        double2 a = s_acc[k][tid];
        for (int tt = 0; tt < nt; ++tt) {
          const double2 xi = s_x[i][tt], xj = s_x[j][tt];
          const double w = s_w[k][tt];
          a.x += w * (xi.x * xj.x + xi.y * xj.y);                    // x_i conj(x_j)
          a.y += w * (xi.y * xj.x - xi.x * xj.y);
        }
        s_acc[k][tid] = a;
      }
  }
  __syncthreads();

  for (int k = 0; k < K; ++k) {                                      // every branch below is block-uniform
    const long long at = (((long long)b * K + k) * N + n) * F + f;
    double2* out = C + at * MM;
    int st = 0;
    if (s_bad[0] | s_bad[1 + k]) st = 1;
    else {
      double tr = 0.0;
      for (int m = 0; m < M; ++m) tr += s_acc[k][m * M + m].x;
      if (tr == 0.0) st = 2;
    }
    double2 c = make_double2(0.0, 0.0);
    if (st == 0 && kind != DOA_MUSIC) {
      if (mine) c = s_acc[k][tid];
    } else if (st == 0) {
      __syncthreads();                                               // the previous class is done with s_A, s_V, s_ord
      if (mine) {
        const double2 r = s_acc[k][tid];
        s_A[i][j][0] = r.x; s_A[i][j][1] = i == j ? 0.0 : r.y;
        if (i != j) { s_A[j][i][0] = r.x; s_A[j][i][1] = -r.y; }
      }
      if (tid < MM) { s_V[i][j][0] = i == j ? 1.0 : 0.0; s_V[i][j][1] = 0.0; }
      __syncthreads();
      jacobi_hermitian<M>(s_A, s_V, tid);
      if (tid < M) s_ord[tid] = tid;
      __syncthreads();
      if (tid < M) {                                                 // descending, equal ones in ascending index
        const double l = s_A[tid][tid][0];
        int rank = 0;
        for (int m = 0; m < M; ++m) {
          const double o = s_A[m][m][0];
          if (o > l || (o == l && m < tid)) ++rank;
        }
        s_ord[rank] = tid;
      }
      __syncthreads();
      const int e0 = s_ord[0], es = s_ord[S - 1];
      if (s_A[es][es][0] <= DOA_RANK_TOL * s_A[e0][e0][0]) st = 2;   // the signal subspace has rank below S
      else if (mine) {
        for (int r = S; r < M; ++r) {
          const int e = s_ord[r];
          const double ar = s_V[i][e][0], ai = s_V[i][e][1], br = s_V[j][e][0], bi = s_V[j][e][1];
          c.x += ar * br + ai * bi;
          c.y += ai * br - ar * bi;
        }
        c.x /= (double)M;
        c.y /= (double)M;
      }
    }
    if (st != 0) c = make_double2(0.0, 0.0);
    if (tid < MM) {
      if (i == j) out[tid] = make_double2(c.x, 0.0);
      else if (i < j) {
        out[tid] = c;
        out[j * M + i] = make_double2(c.x, -c.y);
      }
    }
    if (tid == 0) binst[at] = st;
  }
}

// grid B K N tiles (tile fastest), DOA_TILE threads
template <int M>
__global__ __launch_bounds__(DOA_TILE) void doa_steer_k(const double2* __restrict__ C, const int* __restrict__ binst,
                                                        const double* __restrict__ tau, long long tau_bstride, int KN, int F,
                                                        int D, int tiles, double fs, double nfft, int f_lo, int f_hi, int music,
                                                        double* __restrict__ q) {
  constexpr int NP = M * (M - 1) / 2;
  __shared__ double2 s_c[DOA_CHUNK][NP];
  __shared__ double s_diag[DOA_CHUNK];
  __shared__ int s_use[DOA_CHUNK];
  const int tid = threadIdx.x;
  const long long bkn = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - bkn * tiles);
  const int b = (int)(bkn / KN);
  const int d = tile * DOA_TILE + tid;
  const int dd = d < D ? d : D - 1;
  double tm[M];
  {
    const double* tp = tau + (long long)b * tau_bstride + (long long)dd * M;
#pragma unroll
    for (int m = 0; m < M; ++m) tm[m] = tp[m];
  }
  const double two_pi = 6.283185307179586476925286766559;
  double wr[M], wi[M];                                               // the step from one bin to the next, e^{j (omega_1 - omega_0) tau_m}
#pragma unroll
  for (int m = 0; m < M; ++m) sincos(two_pi * fs / nfft * tm[m], &wi[m], &wr[m]);
  double sum = 0.0;
  int used = 0;
  for (int f0 = f_lo; f0 <= f_hi; f0 += DOA_CHUNK) {
    const int nb = f_hi - f0 + 1 < DOA_CHUNK ? f_hi - f0 + 1 : DOA_CHUNK;
    __syncthreads();
    for (int e = tid; e < nb * NP; e += DOA_TILE) {
      const int bi = e / NP;
      int p = e - bi * NP, m = 0;
      while (p >= M - 1 - m) { p -= M - 1 - m; ++m; }
      s_c[bi][e - bi * NP] = C[((bkn * F + f0 + bi) * M + m) * M + m + 1 + p];
    }
    if (tid < nb) {
      const double2* cf = C + (bkn * F + f0 + tid) * M * M;
      double dg = 0.0;
      for (int m = 0; m < M; ++m) dg += cf[m * M + m].x;
      s_diag[tid] = dg;
      s_use[tid] = binst[bkn * F + f0 + tid] == 0;
    }
    __syncthreads();
    // z_m = e^{j omega_f tau_m}: seeded exactly at the chunk's first bin, then rotated bin by bin (at most DOA_CHUNK - 1 products)
    double zr[M], zi[M];
    {
      const double om = two_pi * (double)f0 * fs / nfft;
#pragma unroll
      for (int m = 0; m < M; ++m) sincos(om * tm[m], &zi[m], &zr[m]);
    }
    for (int bi = 0; bi < nb; ++bi) {
      if (bi) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const double r = zr[m] * wr[m] - zi[m] * wi[m];
          zi[m] = zr[m] * wi[m] + zi[m] * wr[m];
          zr[m] = r;
        }
      }
      if (!s_use[bi]) continue;                                      // block-uniform
      double pr = 0.0;
      int p = 0;
#pragma unroll
      for (int m = 0; m < M - 1; ++m) {
        double yr = 0.0, yi = 0.0;                                   // y = sum_{n > m} C[m,n] conj(z_n)
#pragma unroll
        for (int n = m + 1; n < M; ++n, ++p) {
          const double2 c = s_c[bi][p];
          yr += c.x * zr[n] + c.y * zi[n];
          yi += c.y * zr[n] - c.x * zi[n];
        }
        pr += zr[m] * yr - zi[m] * yi;                               // Re(z_m y)
      }
      sum += s_diag[bi] + 2.0 * pr;
      ++used;
    }
  }
  if (d < D) q[bkn * D + d] = !used ? 0.0 : (music ? sum / (double)used : sum);
}

// grid B K N, DOA_TILE threads
__global__ __launch_bounds__(DOA_TILE) void doa_peak_k(const double* __restrict__ q, const double* __restrict__ pts,
                                                       const int* __restrict__ binst, int F, int D, int S, int music,
                                                       double min_sep2, int* __restrict__ peak, double* __restrict__ value,
                                                       int* __restrict__ fail, int* __restrict__ used_ws,
                                                       int* __restrict__ fail_ws) {
  __shared__ double s_v[DOA_TILE];
  __shared__ int s_i[DOA_TILE];
  __shared__ int s_n[DOA_TILE];
  const int tid = threadIdx.x;
  const long long bkn = blockIdx.x;

  int cnt = 0, nonfin = 0;
  for (int f = tid; f < F; f += DOA_TILE) {
    const int st = binst[bkn * F + f];
    cnt += st == 0;
    nonfin |= st == 1;
  }
  s_n[tid] = cnt;
  s_i[tid] = nonfin;
  __syncthreads();
  for (int h = DOA_TILE / 2; h > 0; h >>= 1) {
    if (tid < h) { s_n[tid] += s_n[tid + h]; s_i[tid] |= s_i[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    const int fl = (s_i[0] ? 1 : 0) | (s_n[0] == 0 ? 2 : 0);
    fail[bkn] = fl;
    fail_ws[bkn] = fl;
    used_ws[bkn] = s_n[0];
  }
  __syncthreads();

  const double* qq = q + bkn * D;
  double px[DOA_MAX_S], py[DOA_MAX_S], pz[DOA_MAX_S];
  int pi[DOA_MAX_S];
#pragma unroll
  for (int r = 0; r < DOA_MAX_S; ++r) { px[r] = py[r] = pz[r] = 0.0; pi[r] = -1; }
#pragma unroll
  for (int r = 0; r < DOA_MAX_S; ++r) {
    if (r < S) {                                                     // block-uniform
      double bv = 0.0;
      int bidx = -1;
      for (int d = tid; d < D; d += DOA_TILE) {
        const double x = pts[3 * d], y = pts[3 * d + 1], z = pts[3 * d + 2];
        bool gone = false;
#pragma unroll
        for (int e = 0; e < DOA_MAX_S; ++e)
          if (e < r && pi[e] >= 0) {
            const double dx = x - px[e], dy = y - py[e], dz = z - pz[e];
            if (d == pi[e] || dx * dx + dy * dy + dz * dz < min_sep2) gone = true;
          }
        if (gone) continue;
        const double v = qq[d];
        if (bidx < 0 || (music ? v < bv : v > bv)) { bv = v; bidx = d; }
      }
      s_v[tid] = bv;
      s_i[tid] = bidx;
      __syncthreads();
      for (int h = DOA_TILE / 2; h > 0; h >>= 1) {
        if (tid < h) {
          const double ov = s_v[tid + h], mv = s_v[tid];
          const int oi = s_i[tid + h], mi = s_i[tid];
          if (oi >= 0 && (mi < 0 || (music ? ov < mv : ov > mv) || (ov == mv && oi < mi))) { s_v[tid] = ov; s_i[tid] = oi; }
        }
        __syncthreads();
      }
      const int best = s_i[0];
      const double bestv = s_v[0];
      __syncthreads();                                               // s_v, s_i are free for the next round
      pi[r] = best;
      if (best >= 0) { px[r] = pts[3 * best]; py[r] = pts[3 * best + 1]; pz[r] = pts[3 * best + 2]; }
      if (tid == 0) {
        peak[bkn * S + r] = best;
        value[bkn * S + r] = best >= 0 ? bestv : 0.0;
      }
    }
  }
}

long long doa_ws_bytes(long long B, long long K, long long N, long long F, long long M) {
  const long long bins = B * K * N * F;
  return bins * M * M * 16 + ((bins * 4 + 15) / 16) * 16 + 2 * ((B * K * N * 4 + 15) / 16) * 16;
}

namespace {
struct DoaWs { double2* C; int* binst; int* used; int* fail; };
DoaWs doa_carve(void* ws, long long B, long long K, long long N, long long F, long long M) {
  char* p = reinterpret_cast<char*>(ws);
  const long long bins = B * K * N * F;
  DoaWs w;
  w.C = reinterpret_cast<double2*>(p);
  p += bins * M * M * 16;
  w.binst = reinterpret_cast<int*>(p);
  p += ((bins * 4 + 15) / 16) * 16;
  w.used = reinterpret_cast<int*>(p);
  p += ((B * K * N * 4 + 15) / 16) * 16;
  w.fail = reinterpret_cast<int*>(p);
  return w;
}

template <int M>
hipError_t doa_launch(const DoaArgs& a, const DoaWs& w, hipStream_t s) {
  const int tiles = (a.D + DOA_TILE - 1) / DOA_TILE;
  const long long bkn = (long long)a.B * a.K * a.N;
  const double nfft = a.F > 1 ? 2.0 * (a.F - 1) : 2.0;
  hipLaunchKernelGGL(doa_cov_k<M>, dim3((unsigned)((long long)a.B * a.N * a.F)), dim3(DOA_FRAMES), 0, s, a.mix, a.weight, a.K, a.N,
                     a.F, a.T, a.block, a.hop, a.f_lo, a.f_hi, a.kind, a.S, w.C, w.binst);
  hipLaunchKernelGGL(doa_steer_k<M>, dim3((unsigned)(bkn * tiles)), dim3(DOA_TILE), 0, s, w.C, w.binst, a.tau,
                     a.Bg == 1 ? 0LL : (long long)a.D * M, a.K * a.N, a.F, a.D, tiles, a.fs, nfft, a.f_lo, a.f_hi,
                     a.kind == DOA_MUSIC ? 1 : 0, a.q);
  hipLaunchKernelGGL(doa_peak_k, dim3((unsigned)bkn), dim3(DOA_TILE), 0, s, a.q, a.pts, w.binst, a.F, a.D, a.S,
                     a.kind == DOA_MUSIC ? 1 : 0, a.min_sep * a.min_sep, a.peak, a.value, a.fail, w.used, w.fail);
  return hipGetLastError();
}
}  // namespace

// the caller (api_array.hip) has checked every limit and the workspace size
hipError_t launch_doa(const DoaArgs& a, void* ws, hipStream_t s) {
  const DoaWs w = doa_carve(ws, a.B, a.K, a.N, a.F, a.M);
  switch (a.M) {
    case 2: return doa_launch<2>(a, w, s);
    case 3: return doa_launch<3>(a, w, s);
    case 4: return doa_launch<4>(a, w, s);
    case 5: return doa_launch<5>(a, w, s);
    case 6: return doa_launch<6>(a, w, s);
    case 7: return doa_launch<7>(a, w, s);
    case 8: return doa_launch<8>(a, w, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_doa_debug(const void* ws, int B, int K, int N, int F, int M, void* c, int* used, int* fail, hipStream_t s) {
  const DoaWs w = doa_carve(const_cast<void*>(ws), B, K, N, F, M);
  const long long bkn = (long long)B * K * N;
  hipError_t e = hipSuccess;
  if (c) e = hipMemcpyAsync(c, w.C, (size_t)(bkn * F * M * M * 16), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && used) e = hipMemcpyAsync(used, w.used, (size_t)(bkn * 4), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && fail) e = hipMemcpyAsync(fail, w.fail, (size_t)(bkn * 4), hipMemcpyDeviceToDevice, s);
  return e;
}

}  // namespace mn
