// Blind separation on the device: auxiliary-function independent vector analysis with iterative source steering (AuxIVA-ISS;
// Ono 2011, Scheibler & Ono 2020) behind a per-bin PCA to K channels, projected back to all microphones by least squares.  C ABI
// misonet_auxiva / misonet_auxiva_debug in api_array.hip; the definition is INTEGRATION.md 4n, restated in NumPy in
// tests/iva_ref.py.  This is the project's own definition in the pyroomacoustics / torchiva family; nothing here was compared
// against those packages.
//
// mix complex64 [B][F][M][T]; everything after the loads is float64.  One launch sequence on the caller's stream:
//
//   iva_pca_k<M>        one workgroup per (b, f): the non-finite check (fail = 1: the bin is all zero from here on), R = X X^H / T
//                       by plain FMAs (LAB.md "Blind separation": everything outside the iterations is 0.4 of the call's
//                       2.4 ms at the bench geometry, and R is computed once), jacobi_hermitian<M>, the K leading eigenvectors
//                       in descending order of their eigenvalues (equal values: the lower index first), each rotated so that
//                       its ref component is real and >= 0 (an eigenvalue <= 1e-12 of the largest counts as 0: its eigenvector is
//                       0, IVA_RANK_TOL), Y = E_K^H X into the workspace
//   per iteration       iva_weights_k: phi[b][k][t] from sum_f |y_k[f, t]|^2 in ascending f -- the cross-bin dependency is the
//                       kernel boundary;
//                       iva_steer_res_k<K> / iva_steer_str_k<K>: one workgroup per (b, f), the K source steps of the bin.  Up to
//                       iva_resident_frames(K) frames the bin's Y and phi stay in registers across the K steps (thread tid owns the
//                       frames tid + n 512 of all K rows: iva_nr(K) of them, 32 doubles of Y and 16 of phi at the most); beyond it
//                       the streaming kernel walks Y in the workspace, 512 frames at a time, twice per source step.  phi y is
//                       never stored.
//   iva_project_k<K>    A[f][m][k] = sum_t x_m conj(y_k) / sum_t |y_k|^2 and the bin's share of power_k
//   iva_order_k         power[b][k] in ascending f, the S strongest rows in descending order (ties: the lower index)
//   iva_image_k         images[b][s][f][m][t] = A[f][m][order_s] y_{order_s}[f][t], rounded once to complex64
//
// 3 + 2 iterations launches (+ 0 host synchronisations): the sequence can be captured in a HIP graph.  Every sum over t is a
// per-thread strided partial, a wave butterfly, then the 8 wave partials added from LDS in wave order; nothing is accumulated with
// atomics and a workgroup never looks at another one's bin: the result is bit-reproducible and depends neither on B nor on the
// position in the batch.  LDS is static and does not grow with T.
#include "kernels.hpp"
#include "cplx.hpp"
#include "stacked_gram.hpp"
#include "jacobi.hpp"

namespace mn {

constexpr int IVA_THREADS = 512;
constexpr int IVA_WAVES = IVA_THREADS / 64;
constexpr int IVA_SMAX = 4;
// An eigenvalue of R that is not above this times the largest counts as 0 -- it is the rounding of the sums, not a direction of
// the data (float32 samples: a genuine component lies above 2^-48 = 3.6e-15 of the largest) -- and its eigenvector and its row
// of Z are 0, as they are in exact arithmetic for a bin of lower rank (T < K, dead or identical microphones).  Without it that
// row is noise of 1e-17 in an arbitrary direction of the null space, which the iterations would scale up to a source.
constexpr double IVA_RANK_TOL = 1e-12;

// frames per thread of the resident steering kernel: K iva_nr(K) <= 16 complex doubles of Y per thread
__host__ __device__ constexpr int iva_nr(int K) { return K <= 1 ? 16 : K == 2 ? 8 : K <= 4 ? 4 : 2; }
int iva_resident_frames(int K) { return iva_nr(K < 1 ? 1 : K > 8 ? 8 : K) * IVA_THREADS; }

// workspace: fail int [B F] | evec c128 [B F][M][K] | A c128 [B F][M][K] | pp double [B F][K] | power double [B][K] |
//            order int [B][4] | phi double [B][K][T] | Y c128 [B F][K][T]
struct IvaWs { long long fail, evec, a, pp, power, order, phi, y, total; };
static IvaWs iva_ws(int B, int K, int F, int M, int T) {
  IvaWs w;
  const long long bins = (long long)B * F;
  w.fail = 0;
  w.evec = sg_align(bins * 4);
  w.a = sg_align(w.evec + bins * M * K * 16);
  w.pp = sg_align(w.a + bins * M * K * 16);
  w.power = sg_align(w.pp + bins * K * 8);
  w.order = sg_align(w.power + (long long)B * K * 8);
  w.phi = sg_align(w.order + (long long)B * IVA_SMAX * 4);
  w.y = sg_align(w.phi + (long long)B * K * T * 8);
  w.total = sg_align(w.y + bins * K * T * 16);
  return w;
}
long long iva_ws_bytes(int B, int K, int F, int M, int T) { return iva_ws(B, K, F, M, T).total; }

// v[i] summed over the workgroup into tot[i], the same bits on every thread: a butterfly per wave, then the wave partials in
// wave order.  red: double [IVA_WAVES NV], tot: double [NV]; two barriers.  The caller alternates between two (red, tot) pairs, so
// that a pair is written again only after two barriers have passed since it was read.
template <int NV>
__device__ __forceinline__ void iva_block_sum(const double (&v)[NV], double* red, double* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double x = v[i];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
    if (lane == 0) red[wave * NV + i] = x;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = red[threadIdx.x];
#pragma unroll
    for (int w = 1; w < IVA_WAVES; ++w) s += red[w * NV + threadIdx.x];
    tot[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---- step 0 and 1: the non-finite check and the PCA.  grid B F, 512 threads
template <int M>
__global__ __launch_bounds__(IVA_THREADS) void iva_pca_k(const float2* mix, int T, int K, int ref, int* fail, double2* evec,
                                                         double2* Y) {
  constexpr int NV = M * M;                          // row i of the lower triangle at i^2: (re, im) of j < i, then the diagonal
  __shared__ double red[IVA_WAVES * NV];
  __shared__ double tot[NV];
  __shared__ double s_A[M][M][2], s_V[M][M][2];
  __shared__ double2 s_E[M][M];                      // [m][k]
  __shared__ int s_idx[M];
  const long long bin = blockIdx.x;
  const int tid = threadIdx.x;
  const float2* x = mix + bin * M * T;

  int bad = 0;
  for (long long e = tid; e < (long long)M * T; e += IVA_THREADS) {
    const float2 v = x[e];
    if (!(fabsf(v.x) <= F32_MAX) || !(fabsf(v.y) <= F32_MAX)) bad = 1;
  }
  bad = __syncthreads_or(bad);

  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0;
  if (!bad)
    for (int t = tid; t < T; t += IVA_THREADS) {
      double xr[M], xi[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float2 v = x[m * T + t];
        xr[m] = (double)v.x;
        xi[m] = (double)v.y;
      }
#pragma unroll
      for (int i = 0; i < M; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) {                // x_i conj(x_j)
          acc[i * i + 2 * j] += xr[i] * xr[j] + xi[i] * xi[j];
          acc[i * i + 2 * j + 1] += xi[i] * xr[j] - xr[i] * xi[j];
        }
        acc[i * i + 2 * i] += xr[i] * xr[i] + xi[i] * xi[i];
      }
    }
  iva_block_sum<NV>(acc, red, tot);
  if (tid < NV) {
    const int i = tid / M, j = tid - i * M;
    const double dT = (double)T;
    if (i == j) {
      s_A[i][i][0] = tot[i * i + 2 * i] / dT;
      s_A[i][i][1] = 0.0;
    } else if (i > j) {
      const double re = tot[i * i + 2 * j] / dT, im = tot[i * i + 2 * j + 1] / dT;
      s_A[i][j][0] = re; s_A[i][j][1] = im;
      s_A[j][i][0] = re; s_A[j][i][1] = -im;
    }
    s_V[i][j][0] = i == j ? 1.0 : 0.0;
    s_V[i][j][1] = 0.0;
  }
  __syncthreads();
  jacobi_hermitian<M>(s_A, s_V, tid);
  __syncthreads();
  if (tid == 0) {                                    // descending eigenvalues, equal ones in ascending index
    unsigned used = 0u;
    for (int k = 0; k < K; ++k) {
      int best = -1;
      for (int i = 0; i < M; ++i)
        if (!(used >> i & 1u) && (best < 0 || s_A[i][i][0] > s_A[best][best][0])) best = i;
      used |= 1u << best;
      s_idx[k] = best;
    }
  }
  __syncthreads();
  if (tid < M * K) {                                 // the ref component real and >= 0
    const int m = tid / K, k = tid - m * K, c = s_idx[k];
    const double er = s_V[ref][c][0], ei = s_V[ref][c][1];
    const double a2 = er * er + ei * ei;
    double rr = 1.0, ri = 0.0;
    if (a2 > 0.0) {
      const double n = sqrt(a2);
      rr = er / n;
      ri = -ei / n;
    }
    const double vr = s_V[m][c][0], vi = s_V[m][c][1];
    const int c0 = s_idx[0];
    const bool live = s_A[c][c][0] > IVA_RANK_TOL * s_A[c0][c0][0];       // else: a direction the bin does not have
    const double2 e = live ? make_double2(vr * rr - vi * ri, vr * ri + vi * rr) : make_double2(0.0, 0.0);
    s_E[m][k] = e;
    evec[(bin * M + m) * K + k] = e;
  }
  __syncthreads();
  double2* y = Y + bin * K * T;
  for (int t = tid; t < T; t += IVA_THREADS) {
    double xr[M], xi[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float2 v = bad ? make_float2(0.f, 0.f) : x[m * T + t];
      xr[m] = (double)v.x;
      xi[m] = (double)v.y;
    }
    for (int k = 0; k < K; ++k) {                    // conj(E[m][k]) x_m, fixed order: microphone 0, 1, ...
      double zr = 0.0, zi = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double2 e = s_E[m][k];
        zr += e.x * xr[m] + e.y * xi[m];
        zi += e.x * xi[m] - e.y * xr[m];
      }
      y[k * T + t] = make_double2(zr, zi);
    }
  }
  if (tid == 0) fail[bin] = bad ? 1 : 0;
}

// ---- step 2: the weights.  grid (B K, ceil(T / 256)), 256 threads: one thread per frame, the bins in ascending order
__global__ __launch_bounds__(256) void iva_weights_k(const double2* Y, int F, int K, int T, int laplace, double floor_,
                                                     double* phi) {
  const int bk = blockIdx.x, b = bk / K, k = bk - b * K;
  const int t = blockIdx.y * 256 + threadIdx.x;
  if (t >= T) return;
  const double2* y = Y + ((long long)b * F * K + k) * T + t;
  double sum = 0.0;
  for (int f = 0; f < F; ++f) {
    const double2 v = y[(long long)f * K * T];
    sum += v.x * v.x + v.y * v.y;
  }
  const double r = laplace ? 2.0 * sqrt(sum) : sum / (double)F;
  phi[(long long)bk * T + t] = 1.0 / fmax(r, floor_);
}

// The sums of source step s over the workgroup and its steps v_k: part [K][3] = this thread's share of (Re num_k, Im num_k, den_k).
// A butterfly per wave, then thread k adds the 8 wave partials of row k in wave order, forms v_k and leaves it in sv [K][2]; a
// non-finite v_k is replaced by 0 and *flag = 2.  red: double [IVA_WAVES 3 K]; two barriers; the caller alternates between two
// (red, sv) pairs, so that a pair is written again only after two barriers have passed since it was read.
template <int K>
__device__ __forceinline__ void iva_step_sum(const double (&part)[3 * K], int s, int T, double* red, double* sv, int* flag) {
  constexpr int NV = 3 * K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double x = part[i];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) x += __shfl_xor(x, k, 64);
    if (lane == 0) red[wave * NV + i] = x;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    double nr = red[3 * k], ni = red[3 * k + 1], den = red[3 * k + 2];
#pragma unroll
    for (int w = 1; w < IVA_WAVES; ++w) {
      nr += red[w * NV + 3 * k];
      ni += red[w * NV + 3 * k + 1];
      den += red[w * NV + 3 * k + 2];
    }
    double vr = 0.0, vi = 0.0;
    if (k != s) {
      if (den != 0.0) {
        vr = nr / den;
        vi = ni / den;
      }
    } else {
      const double d = den / (double)T;
      if (d != 0.0) vr = 1.0 - 1.0 / sqrt(d);
    }
    if (!(fabs(vr) <= F64_MAX) || !(fabs(vi) <= F64_MAX)) {
      vr = vi = 0.0;
      *flag = 2;
    }
    sv[2 * k] = vr;
    sv[2 * k + 1] = vi;
  }
  __syncthreads();
}

// ---- step 3, T <= iva_resident_frames(K): Y and phi of the bin in registers across the K source steps.  grid B F, 512 threads
template <int K>
__global__ __launch_bounds__(IVA_THREADS) void iva_steer_res_k(double2* Y, const double* phi, int F, int T, int* fail) {
  constexpr int NR = iva_nr(K), NV = 3 * K;
  __shared__ double red[2][IVA_WAVES * NV];
  __shared__ double sv[2][2 * K];
  __shared__ int s_flag;
  const long long bin = blockIdx.x;
  const int b = (int)(bin / F), tid = threadIdx.x;
  double2* y = Y + bin * K * T;
  const double* ph = phi + (long long)b * K * T;
  if (tid == 0) s_flag = 0;
  double yr[K][NR], yi[K][NR], w[K][NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int t = tid + n * IVA_THREADS;
    const bool in = t < T;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double2 v = in ? y[k * T + t] : make_double2(0.0, 0.0);
      yr[k][n] = v.x;
      yi[k][n] = v.y;
      w[k][n] = in ? ph[k * T + t] : 0.0;
    }
  }
#pragma unroll
  for (int s = 0; s < K; ++s) {
    double part[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) part[i] = 0.0;
#pragma unroll
    for (int n = 0; n < NR; ++n)
      if (n * IVA_THREADS < T) {                     // the same on every thread
        const double sr = yr[s][n], si = yi[s][n], p2 = sr * sr + si * si;
#pragma unroll
        for (int k = 0; k < K; ++k) {                // phi_k y_k conj(y_s), phi_k |y_s|^2
          const double wk = w[k][n];
          part[3 * k] += wk * (yr[k][n] * sr + yi[k][n] * si);
          part[3 * k + 1] += wk * (yi[k][n] * sr - yr[k][n] * si);
          part[3 * k + 2] += wk * p2;
        }
      }
    iva_step_sum<K>(part, s, T, red[s & 1], sv[s & 1], &s_flag);
    cd v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = {sv[s & 1][2 * k], sv[s & 1][2 * k + 1]};
#pragma unroll
    for (int n = 0; n < NR; ++n)
      if (n * IVA_THREADS < T) {
        const double sr = yr[s][n], si = yi[s][n];   // y_s as it stood before this step
#pragma unroll
        for (int k = 0; k < K; ++k) {
          yr[k][n] -= v[k].re * sr - v[k].im * si;
          yi[k][n] -= v[k].re * si + v[k].im * sr;
        }
      }
  }
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int t = tid + n * IVA_THREADS;
    if (t < T) {
#pragma unroll
      for (int k = 0; k < K; ++k) y[k * T + t] = make_double2(yr[k][n], yi[k][n]);
    }
  }
  if (tid == 0 && s_flag) fail[bin] |= s_flag;            // behind the last step's barriers
}

// ---- step 3, any T: Y stays in the workspace; per source step one pass for the sums and one for the update, 512 frames at a
// time.  A thread reads and writes its own frames only.  grid B F, 512 threads
template <int K>
__global__ __launch_bounds__(IVA_THREADS) void iva_steer_str_k(double2* Y, const double* phi, int F, int T, int* fail) {
  constexpr int NV = 3 * K;
  __shared__ double red[2][IVA_WAVES * NV];
  __shared__ double sv[2][2 * K];
  __shared__ int s_flag;
  const long long bin = blockIdx.x;
  const int b = (int)(bin / F), tid = threadIdx.x;
  double2* y = Y + bin * K * T;
  const double* ph = phi + (long long)b * K * T;
  if (tid == 0) s_flag = 0;
#pragma unroll 1
  for (int s = 0; s < K; ++s) {
    double part[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) part[i] = 0.0;
#pragma unroll 1
    for (int t = tid; t < T; t += IVA_THREADS) {
      const double2 ys = y[s * T + t];
      const double p2 = ys.x * ys.x + ys.y * ys.y;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double2 yk = y[k * T + t];
        const double wk = ph[k * T + t];
        part[3 * k] += wk * (yk.x * ys.x + yk.y * ys.y);
        part[3 * k + 1] += wk * (yk.y * ys.x - yk.x * ys.y);
        part[3 * k + 2] += wk * p2;
      }
    }
    iva_step_sum<K>(part, s, T, red[s & 1], sv[s & 1], &s_flag);
    cd v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = {sv[s & 1][2 * k], sv[s & 1][2 * k + 1]};
#pragma unroll 1
    for (int t = tid; t < T; t += IVA_THREADS) {
      const double2 ys = y[s * T + t];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        double2 yk = y[k * T + t];
        yk.x -= v[k].re * ys.x - v[k].im * ys.y;
        yk.y -= v[k].re * ys.y + v[k].im * ys.x;
        y[k * T + t] = yk;
      }
    }
  }
  if (tid == 0 && s_flag) fail[bin] |= s_flag;            // behind the last step's barriers
}

// ---- step 4: the projection back and the bin's share of the power.  grid B F, 512 threads
template <int K>
__global__ __launch_bounds__(IVA_THREADS) void iva_project_k(const float2* mix, const double2* Y, int M, int T, int ref,
                                                             double2* A, double* pp) {
  constexpr int NV = 2 * K;
  __shared__ double red[2][IVA_WAVES * NV];
  __shared__ double tot[2][NV];
  const long long bin = blockIdx.x;
  const int tid = threadIdx.x;
  const float2* x = mix + bin * M * T;
  const double2* y = Y + bin * K * T;
  double part[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) part[i] = 0.0;
#pragma unroll 1
  for (int t = tid; t < T; t += IVA_THREADS) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double2 v = y[k * T + t];
      part[k] += v.x * v.x + v.y * v.y;
    }
  }
  iva_block_sum<NV>(part, red[0], tot[0]);
  double den[K];
#pragma unroll
  for (int k = 0; k < K; ++k) den[k] = tot[0][k];
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    const int p = (m + 1) & 1;
#pragma unroll
    for (int i = 0; i < NV; ++i) part[i] = 0.0;
#pragma unroll 1
    for (int t = tid; t < T; t += IVA_THREADS) {
      const float2 xf = x[m * T + t];
      const double xr = (double)xf.x, xi = (double)xf.y;
#pragma unroll
      for (int k = 0; k < K; ++k) {                  // x_m conj(y_k)
        const double2 v = y[k * T + t];
        part[2 * k] += xr * v.x + xi * v.y;
        part[2 * k + 1] += xi * v.x - xr * v.y;
      }
    }
    iva_block_sum<NV>(part, red[p], tot[p]);
    if (tid < K) {
      const double d = den[tid];
      double2 a = make_double2(0.0, 0.0);
      if (d != 0.0) a = make_double2(tot[p][2 * tid] / d, tot[p][2 * tid + 1] / d);
      A[(bin * M + m) * K + tid] = a;
      if (m == ref) pp[bin * K + tid] = (a.x * a.x + a.y * a.y) * d;
    }
  }
}

// ---- the power of every row over the bins in ascending order, and the S strongest rows.  grid B, 64 threads
__global__ __launch_bounds__(64) void iva_order_k(const double* pp, int F, int K, int S, double* power, int* order,
                                                  int* order_out) {
  __shared__ double s_p[8];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid < K) {
    double p = 0.0;
    for (int f = 0; f < F; ++f) p += pp[((long long)b * F + f) * K + tid];
    power[b * K + tid] = p;
    s_p[tid] = p;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned used = 0u;
    for (int s = 0; s < IVA_SMAX; ++s) {
      int best = -1;
      if (s < S)
        for (int k = 0; k < K; ++k)
          if (!(used >> k & 1u) && (best < 0 || s_p[k] > s_p[best])) best = k;
      if (best >= 0) used |= 1u << best;
      order[b * IVA_SMAX + s] = best < 0 ? 0 : best;
      if (order_out && s < S) order_out[b * S + s] = best;
    }
  }
}

// ---- the images.  grid (B F, ceil(T / 256)), 256 threads: one thread per frame
__global__ __launch_bounds__(256) void iva_image_k(const double2* Y, const double2* A, const int* order, int F, int M, int K,
                                                   int S, int T, float2* out) {
  const long long bin = blockIdx.x;
  const int b = (int)(bin / F), f = (int)(bin - (long long)b * F);
  const int t = blockIdx.y * 256 + threadIdx.x;
  if (t >= T) return;
  for (int s = 0; s < S; ++s) {
    const int k = order[b * IVA_SMAX + s];
    const double2 v = Y[(bin * K + k) * T + t];
    float2* o = out + ((((long long)b * S + s) * F + f) * M) * T + t;
    for (int m = 0; m < M; ++m) {
      const double2 a = A[(bin * M + m) * K + k];
      o[(long long)m * T] = make_float2((float)(a.x * v.x - a.y * v.y), (float)(a.x * v.y + a.y * v.x));
    }
  }
}

template <int K>
static void iva_launch_k(const IvaArgs& a, const IvaWs& w, char* base, hipStream_t s) {
  const unsigned bins = (unsigned)((long long)a.B * a.F);
  int* fail = reinterpret_cast<int*>(base + w.fail);
  double2* Y = reinterpret_cast<double2*>(base + w.y);
  double* phi = reinterpret_cast<double*>(base + w.phi);
  const bool resident = a.T <= iva_nr(K) * IVA_THREADS;
  for (int it = 0; it < a.iters; ++it) {
    hipLaunchKernelGGL(iva_weights_k, dim3(a.B * K, (a.T + 255) / 256), dim3(256), 0, s, Y, a.F, K, a.T, a.laplace, a.floor, phi);
    if (resident)
      hipLaunchKernelGGL(iva_steer_res_k<K>, dim3(bins), dim3(IVA_THREADS), 0, s, Y, phi, a.F, a.T, fail);
    else
      hipLaunchKernelGGL(iva_steer_str_k<K>, dim3(bins), dim3(IVA_THREADS), 0, s, Y, phi, a.F, a.T, fail);
  }
  hipLaunchKernelGGL(iva_project_k<K>, dim3(bins), dim3(IVA_THREADS), 0, s, reinterpret_cast<const float2*>(a.mix), Y, a.M, a.T,
                     a.ref, reinterpret_cast<double2*>(base + w.a), reinterpret_cast<double*>(base + w.pp));
}

template <int M>
static void iva_launch_pca(const IvaArgs& a, const IvaWs& w, char* base, hipStream_t s) {
  hipLaunchKernelGGL(iva_pca_k<M>, dim3((unsigned)((long long)a.B * a.F)), dim3(IVA_THREADS), 0, s,
                     reinterpret_cast<const float2*>(a.mix), a.T, a.K, a.ref, reinterpret_cast<int*>(base + w.fail),
                     reinterpret_cast<double2*>(base + w.evec), reinterpret_cast<double2*>(base + w.y));
}

hipError_t launch_auxiva(const IvaArgs& a, void* ws, hipStream_t s) {
  if (a.M < 2 || a.M > 8 || a.S < 1 || a.S > IVA_SMAX || a.S > a.K || a.K > a.M || a.T < 1 || a.B < 1 || a.F < 1 ||
      a.iters < 0 || a.ref < 0 || a.ref >= a.M || (long long)a.B * a.F > 0x7fffffffLL || (long long)a.B * a.K > 0x7fffffffLL ||
      (a.T + 255) / 256 > 65535)
    return hipErrorInvalidValue;
  const IvaWs w = iva_ws(a.B, a.K, a.F, a.M, a.T);
  char* base = reinterpret_cast<char*>(ws);
  switch (a.M) {
    case 2: iva_launch_pca<2>(a, w, base, s); break;
    case 3: iva_launch_pca<3>(a, w, base, s); break;
    case 4: iva_launch_pca<4>(a, w, base, s); break;
    case 5: iva_launch_pca<5>(a, w, base, s); break;
    case 6: iva_launch_pca<6>(a, w, base, s); break;
    case 7: iva_launch_pca<7>(a, w, base, s); break;
    default: iva_launch_pca<8>(a, w, base, s); break;
  }
  switch (a.K) {
    case 1: iva_launch_k<1>(a, w, base, s); break;
    case 2: iva_launch_k<2>(a, w, base, s); break;
    case 3: iva_launch_k<3>(a, w, base, s); break;
    case 4: iva_launch_k<4>(a, w, base, s); break;
    case 5: iva_launch_k<5>(a, w, base, s); break;
    case 6: iva_launch_k<6>(a, w, base, s); break;
    case 7: iva_launch_k<7>(a, w, base, s); break;
    default: iva_launch_k<8>(a, w, base, s); break;
  }
  int* order = reinterpret_cast<int*>(base + w.order);
  hipLaunchKernelGGL(iva_order_k, dim3(a.B), dim3(64), 0, s, reinterpret_cast<const double*>(base + w.pp), a.F, a.K, a.S,
                     reinterpret_cast<double*>(base + w.power), order, a.order_out);
  hipLaunchKernelGGL(iva_image_k, dim3((unsigned)((long long)a.B * a.F), (a.T + 255) / 256), dim3(256), 0, s,
                     reinterpret_cast<const double2*>(base + w.y), reinterpret_cast<const double2*>(base + w.a), order, a.F, a.M,
                     a.K, a.S, a.T, reinterpret_cast<float2*>(a.images));
  return hipGetLastError();
}

hipError_t launch_auxiva_debug(const void* ws, int B, int K, int F, int M, int T, void* y, void* a, void* evec, double* power,
                               int* fail, hipStream_t s) {
  const IvaWs w = iva_ws(B, K, F, M, T);
  const char* base = reinterpret_cast<const char*>(ws);
  const long long bins = (long long)B * F;
  hipError_t e = hipSuccess;
  if (y) e = hipMemcpyAsync(y, base + w.y, bins * K * T * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && a) e = hipMemcpyAsync(a, base + w.a, bins * M * K * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && evec) e = hipMemcpyAsync(evec, base + w.evec, bins * M * K * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && power) e = hipMemcpyAsync(power, base + w.power, (long long)B * K * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && fail) e = hipMemcpyAsync(fail, base + w.fail, bins * 4, hipMemcpyDeviceToDevice, s);
  return e;
}

}  // namespace mn
