// Guided spatial clustering on the device: the complex angular central Gaussian mixture model (cACGMM; Ito, Araki & Nakatani
// 2016) of K = S + 1 classes per bin, started from -- and, with the prior "guided", held to -- masks the caller brings (the
// network's).  C ABI misonet_cacgmm / misonet_cacgmm_debug / misonet_masks_from_estimates / misonet_pipeline_set_refine in
// api_array.hip and api_pipeline.hip; the definition is INTEGRATION.md 4l, restated in NumPy in tests/cacgmm_ref.py.
//
// Per (item b, bin f), independent of every other: Y = mix[b, f] [M, T], z[t] = y[t] / |y[t]| (a frame with |y|^2 == 0 is EMPTY:
// it enters no sum and leaves with its initial mask), gamma0 [K, T] the initial masks.
//
//   cacgmm_bin_k   one workgroup of 8 waves per (b, f); iterations + 1 sweeps over the frames, SG_TT at a time through LDS:
//                    z from the staged float32 values, as float64, frame-major [Re z; Im z];
//                    E-step (not in sweep 0: gamma = gamma0, q = 1), thread (class, frame), wave k = class k:
//                      q = |L_k^-1 z|^2 from L_k^-1 in LDS, l = log pi - logdet_k - M log q, gamma = softmax over the classes
//                      through LDS (the maximum subtracted); pi = n_k / sum n_k per bin, or max(gamma0, prior_floor) per frame;
//                    the weights gamma / q into LDS;
//                    M-step (not in the last sweep): wave k adds the tile to ITS 16 x 16 float64 MFMA accumulator, the Gram
//                      matrix of [Re z; Im z] with the weight folded into the B operand (sg_gram_tile1);
//                    after the sweep: n_k, B_k = M / n_k sum (+ diag_load tr / M I), Cholesky B_k = L_k L_k^H by the helpers of
//                      stacked_gram.hpp, logdet_k, L_k^-1 column by column, pi;
//                    the last sweep writes the masks and the images gamma_s Y
//   masks_from_est_k   the initial masks from S source estimates and the mixture, one thread per (b, f, t)
//
// Every sum runs in a fixed order -- the MFMA chain tile by tile in ascending t; n_k and the log-likelihood as per-lane sums in
// ascending t, joined by one butterfly -- nothing is accumulated with atomics and a workgroup never looks at another one: the
// result is bit-reproducible and depends neither on B nor on the position in the batch.  A bin whose n_k is not > 0 or not
// finite, whose Cholesky meets a pivot that is not finite or not > 0, or whose log-likelihood is not finite is UNSOLVED: it
// leaves with its initial masks and their images, fail = 1, and skips its remaining sweeps.  Nothing is clamped.
//
// Limits: 2 <= M <= 8 (2 M <= 16 rows: one tile), 2 <= K <= 5 (one wave per class).  38 KB of static LDS, nothing that grows with T.
#include "kernels.hpp"
#include "cplx.hpp"
#include "stacked_gram.hpp"

namespace mn {

constexpr int CG_KMAX = 5;            // classes: four speakers and the noise
constexpr int CG_ZP = 17;             // pitch of a frame's 16 rows of z, in doubles (odd)

// workspace: fail int [B F] | ll double [B F] | pi double [B F][K] | B_k c128 [B F][K][M][M]
struct CgWs { long long fail, ll, pi, bk, total; };
__host__ __device__ inline CgWs cg_ws(int B, int K, int F, int M) {
  CgWs w;
  const long long bins = (long long)B * F;
  w.fail = 0;
  w.ll = sg_align(bins * 4);
  w.pi = sg_align(w.ll + bins * 8);
  w.bk = sg_align(w.pi + bins * K * 8);
  w.total = sg_align(w.bk + bins * K * M * M * 16);
  return w;
}
long long cacgmm_ws_bytes(int B, int K, int F, int M) { return cg_ws(B, K, F, M).total; }

// grid (F, B), 512 threads
__global__ __launch_bounds__(SG_THREADS) void cacgmm_bin_k(const CacgmmArgs a, int* fail_out, double* ll_out, double* pi_out,
                                                           double2* bk_out) {
  __shared__ float ywin[16 * SG_TT];                // [2 M][TT]: the staged observation, real rows then imaginary rows
  __shared__ double zt[SG_TT * CG_ZP];              // [TT][16 (+ 1)]: [Re z; Im z] of a frame, the rows past 2 M zero
  __shared__ double ell[CG_KMAX * SG_TT];           // [K][TT]: the log-posteriors before the softmax
  __shared__ double wt[CG_KMAX * SG_TT];            // [K][TT]: gamma / q, 0 for an empty frame
  __shared__ double gs[CG_KMAX * 256];              // [K][16][16]: the Gram tiles after a sweep
  __shared__ double2 P[CG_KMAX * 64];               // [K][M][M]: B_k (lower triangle), then its factor L_k
  __shared__ double2 Li[CG_KMAX * 64];              // [K][M][M]: L_k^-1 (lower triangle)
  __shared__ double2 col[8];
  __shared__ double red[SG_WAVES];
  __shared__ double nk[CG_KMAX], logdet[CG_KMAX], logpi[CG_KMAX];
  __shared__ double llsum;
  __shared__ int live[SG_TT];                       // the frame is not empty
  const int M = a.M, T = a.T, K = a.K, S = K - 1;
  const int f = blockIdx.x, b = blockIdx.y;
  const long long bin = (long long)b * a.F + f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  const long long yoff = (long long)b * a.mix.sb + (long long)f * a.mix.sf;
  const float* yre = a.mix.re + yoff;
  const float* yim = a.mix.im + yoff;
  const long long yst = a.mix.st;
  const auto load_y = [&](int m, int t) {
    return make_float2(yre[(long long)m * a.mix.sm + t * yst], yim[(long long)m * a.mix.sm + t * yst]);
  };
  const long long kstride = (long long)a.F * T;                        // masks [B][K][F][T]
  const long long moff = ((long long)b * K * a.F + f) * T;
  const float* init = a.init + moff;
  float* mout = a.masks + moff;
  const long long ioff = (long long)b * a.img.sb + (long long)f * a.img.sf;
  const int ntile_t = (T + SG_TT - 1) / SG_TT;
  const double dM = (double)M;
  const int k = wave;                                                  // thread (class, frame) of the E-step: wave k = class k

  // sweep s = 0 .. iters: the E-step from s = 1 on, the M-step up to s = iters - 1, the outputs at s = iters.  `ident`: the sweep
  // of an unsolved bin, which writes the initial masks and their images.  Every condition below is the same on every thread
  int s = 0;
  bool ident = false, failed = false;
  double ll = 0.0;
  while (true) {
    const bool do_e = !ident && s > 0, do_gram = !ident && s < a.iters, write = ident || s == a.iters;
    d4 acc = d4{0.0, 0.0, 0.0, 0.0};
    double n_acc = 0.0, ll_acc = 0.0;
#pragma unroll 1
    for (int tt = 0; tt < ntile_t; ++tt) {
      const int t0 = tt * SG_TT, t = t0 + lane;
      __syncthreads();                                                 // the tile before is consumed, the M-step is finished
      sg_stage_rows(load_y, M, T, t0, ywin);
      __syncthreads();
      // ---- z = y / |y| (the frames past T are staged as zeros: empty)
      for (int e = tid; e < SG_TT * 16; e += SG_THREADS) {
        const int tl = e >> 4, r = e & 15;
        double p = 0.0;
        for (int m = 0; m < M; ++m) {                                  // fixed order: microphone 0, 1, ...
          const double xr = (double)ywin[m * SG_TT + tl], xi = (double)ywin[(M + m) * SG_TT + tl];
          p = fma(xr, xr, p);
          p = fma(xi, xi, p);
        }
        const bool on = p > 0.0;
        zt[tl * CG_ZP + r] = on && r < 2 * M ? (double)ywin[r * SG_TT + tl] / sqrt(p) : 0.0;
        if (r == 0) live[tl] = on ? 1 : 0;
      }
      __syncthreads();
      // ---- the E-step
      bool on = false;
      float g0f = 0.f;
      double q = 1.0;
      if (k < K) {
        on = live[lane] != 0;
        if (t < T) g0f = init[k * kstride + t];
        if (do_e) {
          double l = 0.0;
          if (on) {
            const double2* Lk = Li + k * 64;
            const double* z = zt + lane * CG_ZP;
            q = 0.0;
            for (int i = 0; i < M; ++i) {                              // row i of L_k^-1 z
              double ar = 0.0, ai = 0.0;
              for (int j = 0; j <= i; ++j) {
                const double2 lv = Lk[i * M + j];
                const double zr = z[j], zi = z[M + j];
                ar += lv.x * zr - lv.y * zi;
                ai += lv.x * zi + lv.y * zr;
              }
              q += ar * ar + ai * ai;
            }
            const double lp = a.guided ? log(fmax((double)g0f, a.prior_floor)) : logpi[k];
            l = lp - logdet[k] - dM * log(q);
          }
          ell[k * SG_TT + lane] = l;
        }
      }
      if (do_e) __syncthreads();
      if (k < K) {
        double gam = (double)g0f;
        if (do_e && on) {
          double mx = ell[lane];
          for (int c = 1; c < K; ++c) mx = fmax(mx, ell[c * SG_TT + lane]);
          double sum = 0.0;
          for (int c = 0; c < K; ++c) sum += exp(ell[c * SG_TT + lane] - mx);       // fixed order: class 0, 1, ...
          gam = exp(ell[k * SG_TT + lane] - mx) / sum;
          if (k == 0) ll_acc += mx + log(sum);
        }
        wt[k * SG_TT + lane] = on ? gam / q : 0.0;
        if (on) n_acc += gam;
        if (write) {
          if (t < T) mout[k * kstride + t] = on ? (float)gam : g0f;    // an empty frame keeps its initial mask, bit for bit
          if (a.img.re && k < S && t < a.img.Tp) {                     // gamma_s Y, rounded once; zeros in [T, Tp)
            const long long o = ioff + (long long)k * a.img.ss + (long long)t * a.img.st;
            for (int m = 0; m < M; ++m) {
              const double yr = (double)ywin[m * SG_TT + lane], yi = (double)ywin[(M + m) * SG_TT + lane];
              a.img.re[o + m * a.img.sm] = t < T ? (float)(gam * yr) : 0.f;
              a.img.im[o + m * a.img.sm] = t < T ? (float)(gam * yi) : 0.f;
            }
          }
        }
      }
      __syncthreads();
      // ---- the M-step's sum: the Gram tile of class k on wave k
      if (do_gram && k < K) sg_gram_tile1(acc, zt, CG_ZP, wt + k * SG_TT);
    }
    if (ident) break;

    if (do_e) {                                                        // the log-likelihood of this E-step
      if (wave == 0) {
        const double v = wave_sum(ll_acc);
        if (lane == 0) llsum = v;
      }
      __syncthreads();
      ll = llsum;
      if (!finite(ll)) { failed = ident = true; continue; }
    }
    if (!do_gram) break;

    // ---- the M-step: n_k, B_k, its factor, logdet_k, L_k^-1, pi
    if (k < K) {
      const double v = wave_sum(n_acc);
      if (lane == 0) nk[k] = v;
#pragma unroll
      for (int r = 0; r < 4; ++r) gs[k * 256 + (lg + 4 * r) * 16 + lr] = acc[r];
    }
    __syncthreads();
    bool bad = false;
    double ntot = 0.0;
    for (int c = 0; c < K; ++c) {
      const double v = nk[c];
      if (!(v > 0.0) || !(v <= F64_MAX)) bad = true;
      ntot += v;
    }
    if (bad) { failed = ident = true; continue; }
    for (int e = tid; e < K * M * M; e += SG_THREADS) {
      const int c = e / (M * M), r = e - c * M * M, i = r / M, j = r - i * M;
      if (i >= j) {
        const double2 v = sg_tile1_entry(gs + c * 256, M, i, j);
        const double sc = dM / nk[c];
        P[c * 64 + i * M + j] = make_double2(sc * v.x, sc * v.y);
      }
    }
#pragma unroll 1
    for (int c = 0; c < K; ++c) {
      double2* Pc = P + c * 64;
      __syncthreads();
      if (a.diag_load != 0.0) {
        sg_diag_load(Pc, M, a.diag_load, red);
        __syncthreads();
      }
      for (int e = tid; e < M * M; e += SG_THREADS) {                  // B_k as it is factored, the whole Hermitian matrix
        const int i = e / M, j = e - i * M;
        double2 v = i >= j ? Pc[i * M + j] : Pc[j * M + i];
        if (i < j) v.y = -v.y;
        bk_out[(bin * K + c) * M * M + e] = v;
      }
      __syncthreads();
      if (!sg_cholesky(Pc, M, M, col)) { bad = true; break; }
    }
    if (bad) { failed = ident = true; continue; }
    if (tid < K) {
      double ld = 0.0;
      for (int i = 0; i < M; ++i) ld += log(P[tid * 64 + i * M + i].x);
      logdet[tid] = 2.0 * ld;
      const double pk = nk[tid] / ntot;
      logpi[tid] = log(pk);
      pi_out[bin * K + tid] = pk;
    }
    if (tid < K * M) {                                                 // column c of L_k^-1 by forward substitution
      const int kk = tid / M, c = tid - kk * M;
      const double2* Lk = P + kk * 64;
      double2* X = Li + kk * 64;
      for (int i = c; i < M; ++i) {
        double2 v = make_double2(i == c ? 1.0 : 0.0, 0.0);
        for (int j = c; j < i; ++j) {
          const double2 lv = Lk[i * M + j], x = X[j * M + c];
          v.x -= lv.x * x.x - lv.y * x.y;
          v.y -= lv.x * x.y + lv.y * x.x;
        }
        const double d = Lk[i * M + i].x;
        X[i * M + c] = make_double2(v.x / d, v.y / d);
      }
    }
    ++s;
  }

  if (tid == 0) {
    fail_out[bin] = failed ? 1 : 0;
    ll_out[bin] = failed ? 0.0 : ll;
  }
  if (failed || a.iters == 0) {                                        // nothing was estimated: zeros
    for (int e = tid; e < K; e += SG_THREADS) pi_out[bin * K + e] = 0.0;
    for (int e = tid; e < K * M * M; e += SG_THREADS) bk_out[bin * K * M * M + e] = make_double2(0.0, 0.0);
  }
}

// grid (ceil(T / 256), F, B), 256 threads: one thread per frame
__global__ __launch_bounds__(256) void masks_from_est_k(const MaskArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
  if (t >= a.T) return;
  const int S = a.S, K = S + 1;
  double p[4] = {0.0, 0.0, 0.0, 0.0};
  double pn = 0.0;
  const long long yoff = (long long)b * a.mix.sb + (long long)f * a.mix.sf + (long long)t * a.mix.st;
  for (int m = 0; m < a.M; ++m) {                                      // fixed order: microphone 0, 1, ...; speaker 0, 1, ...
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (s < S) {
        const float *re, *im;
        int st;
        src_row(a, b, f, m, s, re, im, st);
        const long long o = (a.est ? 0 : (long long)s * a.src_ss) + (long long)t * st;
        const double xr = (double)re[o], xi = (double)im[o];
        p[s] = fma(xr, xr, p[s]);
        p[s] = fma(xi, xi, p[s]);
        sr += xr;
        si += xi;
      }
    const double dr = (double)a.mix.re[yoff + (long long)m * a.mix.sm] - sr;
    const double di = (double)a.mix.im[yoff + (long long)m * a.mix.sm] - si;
    pn = fma(dr, dr, pn);
    pn = fma(di, di, pn);
  }
  double tot = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < S) tot += p[s];
  tot += pn;
  float* o = a.masks + ((long long)b * K * a.F + f) * a.T + t;
  const long long kstride = (long long)a.F * a.T;
  const bool any = tot > 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (s < S) o[s * kstride] = (float)(any ? p[s] / tot : 1.0 / (double)K);
  o[S * kstride] = (float)(any ? pn / tot : 1.0 / (double)K);
}

hipError_t launch_cacgmm(const CacgmmArgs& a, void* ws, hipStream_t s) {
  if (a.M < 2 || a.M > 8 || a.K < 2 || a.K > CG_KMAX || a.T < 1 || a.iters < 0 || a.B < 1 || a.B > 65535 || a.F < 1)
    return hipErrorInvalidValue;
  const CgWs w = cg_ws(a.B, a.K, a.F, a.M);
  char* base = reinterpret_cast<char*>(ws);
  hipLaunchKernelGGL(cacgmm_bin_k, dim3(a.F, a.B), dim3(SG_THREADS), 0, s, a, reinterpret_cast<int*>(base + w.fail),
                     reinterpret_cast<double*>(base + w.ll), reinterpret_cast<double*>(base + w.pi),
                     reinterpret_cast<double2*>(base + w.bk));
  return hipGetLastError();
}

hipError_t launch_cacgmm_debug(const void* ws, int B, int K, int F, int M, void* bk, double* pi, double* ll, int* fail,
                               hipStream_t s) {
  const CgWs w = cg_ws(B, K, F, M);
  const char* base = reinterpret_cast<const char*>(ws);
  const long long bins = (long long)B * F;
  hipError_t e = hipSuccess;
  if (bk) e = hipMemcpyAsync(bk, base + w.bk, bins * K * M * M * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && pi) e = hipMemcpyAsync(pi, base + w.pi, bins * K * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && ll) e = hipMemcpyAsync(ll, base + w.ll, bins * 8, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && fail) e = hipMemcpyAsync(fail, base + w.fail, bins * 4, hipMemcpyDeviceToDevice, s);
  return e;
}

hipError_t launch_masks_from_est(const MaskArgs& a, hipStream_t s) {
  if (a.S < 1 || a.S > 4 || a.M < 1 || a.T < 1 || a.B < 1 || a.B > 65535 || a.F < 1 || a.F > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(masks_from_est_k, dim3((a.T + 255) / 256, a.F, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mn
