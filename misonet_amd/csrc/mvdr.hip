// MVDR beamformer (reference tester.py:1071-1136, 1138-1167, 1211-1228) and PIT speaker alignment
// (tester.py:1043-1065, 889-915) as an HBM-bound batched small-matrix path: one workgroup per (utterance, bin,
// speaker) streams the M x T slabs once, accumulates both spatial covariance matrices in registers, reduces them
// across the wavefronts, and solves the M x M Hermitian eigenproblem in float64 (cyclic complex Jacobi).
//
//   k1 mvdr_scm_eig : Phi_s = S S^H / T, Phi_n = (Y-S)(Y-S)^H / T  (tester.py:1091-1100, 1138-1152)
//                     principal eigenvector of Phi_s                 (tester.py:1107-1115)
//                     d <- d / d[0];  d <- d * sqrt(M / ||d||_2)      (tester.py:1119-1123; norm, not norm^2)
//   k2 mvdr_solve   : sequential-in-f phase correction               (tester.py:1154-1167)
//                     w = (Phi_n + eps I)^-1 d / (d^H (Phi_n + eps I)^-1 d)   (tester.py:1211-1225)
//   k3 mvdr_apply   : out[t] = sum_m conj(w_m) Y_m[t]                (tester.py:1227-1228)
// The other beamformers (misonet_bf_opts) share k1 and k3: k1 takes Phi_n from Y instead of Y - S for noise = mix
// (tester.py:1096) and, for souden / gev, writes Phi_s beside Phi_n and leaves the eigen-solve out (bf_scm: the same body with MIX);
//   k2' bf_solve    : one wave per (b, spk, f), no dependence from bin to bin: Phi_n' (conditioning, trace normalisation,
//                     eps I), Cholesky Phi_n' = L L^H, souden w = (Phi_n'^-1 Phi_s)[:, ref] / tr or gev C = L^-1 Phi_s L^-H,
//                     Jacobi, w = L^-H u with the phase fixed per bin; blind analytic normalisation (tester.py:1186-1208)
#include "kernels.hpp"
#include "jacobi.hpp"

namespace mn {


// workspace layout (doubles): steer0 [B][S][F][M][2] | phin [B][S][F][M][M][2] | steer1 [B][S][F][M][2] | w [B][S][F][M][2]
__host__ __device__ inline long long ws_steer0(int B, int S, int F, int M) { return 0; }
__host__ __device__ inline long long ws_phin(int B, int S, int F, int M) { return (long long)B * S * F * M * 2; }
__host__ __device__ inline long long ws_steer1(int B, int S, int F, int M) {
  return ws_phin(B, S, F, M) + (long long)B * S * F * M * M * 2;
}
__host__ __device__ inline long long ws_w(int B, int S, int F, int M) {
  return ws_steer1(B, S, F, M) + (long long)B * S * F * M * 2;
}
long long mvdr_ws_bytes(int B, int S, int F, int M) {
  return (ws_w(B, S, F, M) + (long long)B * S * F * M * 2) * (long long)sizeof(double);
}
// souden / gev append: phis [B][S][F][M][M][2] | lam [B][S][F]
__host__ __device__ inline long long ws_phis(int B, int S, int F, int M) {
  return ws_w(B, S, F, M) + (long long)B * S * F * M * 2;
}
__host__ __device__ inline long long ws_lam(int B, int S, int F, int M) {
  return ws_phis(B, S, F, M) + (long long)B * S * F * M * M * 2;
}
long long bf_ws_bytes(int B, int S, int F, int M, int kind) {
  if (kind == BF_MVDR) return mvdr_ws_bytes(B, S, F, M);
  return (ws_lam(B, S, F, M) + (long long)B * S * F) * (long long)sizeof(double);
}


// For souden and gev (a.kind, uniform) Phi_s goes to the workspace beside Phi_n and the eigen-solve is left to bf_solve.
// bf_scm is the same kernel with Phi_n from the observation itself (MIX: MPDR, tester.py:1096).
template <int M>
__global__ __launch_bounds__(256) void mvdr_scm_eig(const MvdrArgs a, double* ws) {
  constexpr bool MIX = false;
#include "mvdr_scm_body.inc"
}
template <int M>
__global__ __launch_bounds__(256) void bf_scm(const MvdrArgs a, double* ws) {
  constexpr bool MIX = true;
#include "mvdr_scm_body.inc"
}

// Phi_n' of one bin from the stored Phi_n [M][M][2]: conditioning (Phi_n + gamma tr / M I) / (1 + gamma), then the division by
// the trace of that (tester.py:1099), then eps I (tester.py:1221).  With gamma = 0 and no trace normalisation every step but
// the last is exact (+ 0, / 1).
struct PhinPrime {
  double add, div1, div2, eps;
  template <int M>
  __device__ inline void init(const double* pn, double cond, int tn, double epsi) {
    double tr = 0.0;
    for (int k = 0; k < M; ++k) tr += pn[(k * M + k) * 2];
    add = cond * tr / (double)M;
    div1 = 1.0 + cond;
    div2 = 1.0;
    if (tn) {
      double t2 = 0.0;
      for (int k = 0; k < M; ++k) t2 += (pn[(k * M + k) * 2] + add) / div1;
      div2 = t2;
    }
    eps = epsi;
  }
  template <int M>
  __device__ inline cd at(const double* pn, int i, int j) const {
    cd v = {pn[(i * M + j) * 2], pn[(i * M + j) * 2 + 1]};
    if (i == j) v.re += add;
    v.re = v.re / div1 / div2;
    v.im = v.im / div1 / div2;
    if (i == j) v.re += eps;
    return v;
  }
};

// blind analytic normalisation (tester.py:1196-1208, eps = 0): w <- w sqrt|w^H N N w| / |w^H N w| with N = Phi_n' Hermitian,
// so w^H N N w = ||N w||^2; a zero denominator leaves w as it is.  N(i, j) returns element (i, j).
template <int M, class NF>
__device__ inline void ban_scale(cd (&w)[M], NF N) {
  cd den = {0.0, 0.0};
  double num = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    cd v = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < M; ++j) v = cadd(v, cmul(N(i, j), w[j]));
    num += cabs2(v);
    den = cadd(den, cmul(cconj(w[i]), v));
  }
  const double d = sqrt(cabs2(den));
  if (d == 0.0) return;
  const double g = sqrt(num) / d;
#pragma unroll
  for (int i = 0; i < M; ++i) { w[i].re *= g; w[i].im *= g; }
}

// one workgroup per (b, spk): thread 0 runs the sequential phase correction over f, then thread f solves bin f.
// mvdr_solve_ext compiles in the options beyond the reference's live path: conditioning, trace normalisation, BAN.
template <int M>
__global__ __launch_bounds__(256) void mvdr_solve(int B, int S, int F, double epsi, double* ws) {
  constexpr bool EXT = false;
  constexpr double cond = 0.0;
  constexpr int tn = 0, ban = 0;
#include "mvdr_solve_body.inc"
}
template <int M>
__global__ __launch_bounds__(256) void mvdr_solve_ext(int B, int S, int F, double epsi, double* ws, double cond, int tn,
                                                      int ban) {
  constexpr bool EXT = true;
#include "mvdr_solve_body.inc"
}

// souden / gev: one single-wave workgroup per (b, spk, f), as mvdr_scm_eig -- nothing depends on another bin.  All float64.
//   N = Phi_n' (PhinPrime), Cholesky N = L L^H: column j by lane j (diagonal) and lanes i > j (below it).  A pivot <= 0 gives
//   sqrt(< 0) = NaN or a division by 0: the non-finite w is what the caller sees, nothing is clamped.
//   X = L^-1 Phi_s: lane j owns column j (forward substitution).
//   souden: G = L^-H X, again a column per lane; w = G[:, ref] / tr(G), 0 where tr(G) == 0.
//   gev:    C = X L^-H = (L^-1 X^H)^H, lane j owns row j; Jacobi on C; w = L^-H u, w^H N w = 1,
//           (N w)[ref] real and >= 0; lambda_max beside it.
template <int M, int KIND>
__global__ __launch_bounds__(64) void bf_solve(int B, int S, int F, double epsi, double cond, int tn, int ban, int ref,
                                               double* ws) {
  __shared__ double s_N[M][M][2];
  __shared__ double s_L[M][M][2];
  __shared__ double s_A[M][M][2];
  __shared__ double s_C[M][M][2];
  __shared__ double s_V[M][M][2];
  const int f = blockIdx.x, b = blockIdx.y, spk = blockIdx.z;
  const int tid = threadIdx.x;
  const long long idx = ((long long)(b * S + spk) * F + f);
  const double* pn = ws + ws_phin(B, S, F, M) + idx * (M * M * 2);
  const double* ps = ws + ws_phis(B, S, F, M) + idx * (M * M * 2);
  PhinPrime P;
  P.init<M>(pn, cond, tn, epsi);
  for (int e = tid; e < M * M; e += 64) {
    const int i = e / M, j = e - i * M;
    const cd v = P.at<M>(pn, i, j);
    s_N[i][j][0] = v.re; s_N[i][j][1] = v.im;
    s_A[i][j][0] = ps[e * 2]; s_A[i][j][1] = ps[e * 2 + 1];
    s_L[i][j][0] = 0.0; s_L[i][j][1] = 0.0;
    s_V[i][j][0] = (i == j) ? 1.0 : 0.0; s_V[i][j][1] = 0.0;
  }
  __syncthreads();
  for (int j = 0; j < M; ++j) {                            // Cholesky, left-looking: column j from the columns before it
    if (tid == j) {
      double d = s_N[j][j][0];
      for (int k = 0; k < j; ++k) d -= s_L[j][k][0] * s_L[j][k][0] + s_L[j][k][1] * s_L[j][k][1];
      s_L[j][j][0] = sqrt(d);                              // d <= 0: NaN, or a division by zero below
    }
    __syncthreads();
    if (tid > j && tid < M) {
      const int i = tid;
      cd acc = {s_N[i][j][0], s_N[i][j][1]};
      for (int k = 0; k < j; ++k)
        acc = csub(acc, cmulc(cd{s_L[i][k][0], s_L[i][k][1]}, cd{s_L[j][k][0], s_L[j][k][1]}));
      const double ljj = s_L[j][j][0];
      s_L[i][j][0] = acc.re / ljj; s_L[i][j][1] = acc.im / ljj;
    }
    __syncthreads();
  }
  if (tid < M) {                                           // X = L^-1 Phi_s, column tid, in place
    const int j = tid;
    for (int i = 0; i < M; ++i) {
      cd acc = {s_A[i][j][0], s_A[i][j][1]};
      for (int k = 0; k < i; ++k) acc = csub(acc, cmul(cd{s_L[i][k][0], s_L[i][k][1]}, cd{s_A[k][j][0], s_A[k][j][1]}));
      const double lii = s_L[i][i][0];
      s_A[i][j][0] = acc.re / lii; s_A[i][j][1] = acc.im / lii;
    }
  }
  __syncthreads();
  cd w[M];
  double lam = 0.0;
  if constexpr (KIND == BF_SOUDEN) {
    if (tid < M) {                                         // G = L^-H X, column tid, in place
      const int j = tid;
      for (int i = M - 1; i >= 0; --i) {
        cd acc = {s_A[i][j][0], s_A[i][j][1]};
        for (int k = i + 1; k < M; ++k)                    // (L^H)[i][k] = conj(L[k][i])
          acc = csub(acc, cmul(cconj(cd{s_L[k][i][0], s_L[k][i][1]}), cd{s_A[k][j][0], s_A[k][j][1]}));
        const double lii = s_L[i][i][0];
        s_A[i][j][0] = acc.re / lii; s_A[i][j][1] = acc.im / lii;
      }
    }
    __syncthreads();
    if (tid != 0) return;
    cd tr = {0.0, 0.0};
    for (int i = 0; i < M; ++i) tr = cadd(tr, cd{s_A[i][i][0], s_A[i][i][1]});
    const bool zero = tr.re == 0.0 && tr.im == 0.0;
    for (int i = 0; i < M; ++i) w[i] = zero ? cd{0.0, 0.0} : cdiv(cd{s_A[i][ref][0], s_A[i][ref][1]}, tr);
  } else {
    if (tid < M) {                                         // row tid of C: solve L c = conj(X[tid, :])^T, C[tid][i] = conj(c_i)
      const int r = tid;
      cd c[M];
      for (int i = 0; i < M; ++i) {
        cd acc = {s_A[r][i][0], -s_A[r][i][1]};
        for (int k = 0; k < i; ++k) acc = csub(acc, cmul(cd{s_L[i][k][0], s_L[i][k][1]}, c[k]));
        const double lii = s_L[i][i][0];
        c[i] = {acc.re / lii, acc.im / lii};
        s_C[r][i][0] = c[i].re; s_C[r][i][1] = -c[i].im;
      }
    }
    __syncthreads();
    for (int e = tid; e < M * M; e += 64) {                // Hermitian part of C (it is Hermitian up to rounding)
      const int i = e / M, j = e - i * M;
      s_A[i][j][0] = 0.5 * (s_C[i][j][0] + s_C[j][i][0]);
      s_A[i][j][1] = (i == j) ? 0.0 : 0.5 * (s_C[i][j][1] - s_C[j][i][1]);
    }
    __syncthreads();
    jacobi_hermitian<M>(s_A, s_V, tid);
    if (tid != 0) return;
    int best = 0;                                          // largest eigenvalue, first on ties
    for (int i = 1; i < M; ++i)
      if (s_A[i][i][0] > s_A[best][best][0]) best = i;
    lam = s_A[best][best][0];
    for (int i = M - 1; i >= 0; --i) {                     // w = L^-H u
      cd acc = {s_V[i][best][0], s_V[i][best][1]};
      for (int k = i + 1; k < M; ++k) acc = csub(acc, cmul(cconj(cd{s_L[k][i][0], s_L[k][i][1]}), w[k]));
      const double lii = s_L[i][i][0];
      w[i] = {acc.re / lii, acc.im / lii};
    }
    cd nref = {0.0, 0.0};                                  // (N w)[ref], and q = w^H N w
    double q = 0.0;
    for (int i = 0; i < M; ++i) {
      cd v = {0.0, 0.0};
      for (int j = 0; j < M; ++j) v = cadd(v, cmul(cd{s_N[i][j][0], s_N[i][j][1]}, w[j]));
      q += w[i].re * v.re + w[i].im * v.im;
      if (i == ref) nref = v;
    }
    const double sc = 1.0 / sqrt(q);
    const double az = sqrt(cabs2(nref));
    cd rot = {sc, 0.0};                                    // scale, and the rotation that makes (N w)[ref] real and >= 0
    if (az > 0.0) rot = {sc * nref.re / az, -sc * nref.im / az};
    for (int i = 0; i < M; ++i) w[i] = cmul(w[i], rot);
  }
  if (ban) ban_scale<M>(w, [&](int i, int j) { return cd{s_N[i][j][0], s_N[i][j][1]}; });
  double* wo = ws + ws_w(B, S, F, M) + idx * (M * 2);
  for (int i = 0; i < M; ++i) {
    wo[i * 2] = w[i].re;
    wo[i * 2 + 1] = w[i].im;
  }
  if (KIND == BF_GEV) ws[ws_lam(B, S, F, M) + idx] = lam;
}

template <int M>
__global__ __launch_bounds__(256) void mvdr_apply(const MvdrArgs a, const COut out, const double* ws) {
  const int f = blockIdx.x, b = blockIdx.y, spk = blockIdx.z;
  const double* wp = ws + ws_w(a.B, a.S, a.F, M) + ((long long)(b * a.S + spk) * a.F + f) * (M * 2);
  float wr[M], wi[M];
  const float *yre[M], *yim[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    wr[m] = (float)wp[m * 2];
    wi[m] = (float)wp[m * 2 + 1];
    const long long off = (long long)b * a.mix.sb + (long long)f * a.mix.sf + (long long)m * a.mix.sm;
    yre[m] = a.mix.re + off;
    yim[m] = a.mix.im + off;
  }
  const int yst = a.mix.st;
  float* ore = out.re + (long long)b * out.ob + (long long)spk * out.os + (long long)f * out.of;
  float* oim = out.im + (long long)b * out.ob + (long long)spk * out.os + (long long)f * out.of;
  for (int t = threadIdx.x; t < a.T; t += 256) {
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float yr = yre[m][(long long)t * yst], yi = yim[m][(long long)t * yst];
      re += wr[m] * yr + wi[m] * yi;                      // conj(w) * y
      im += wr[m] * yi - wi[m] * yr;
    }
    ore[(long long)t * out.ot] = re;
    oim[(long long)t * out.ot] = im;
  }
}

template <int M, bool MIX>
static hipError_t bf_run(const MvdrArgs& a, const COut& out, double* ws, hipStream_t s) {
  dim3 g(a.F, a.B, a.S);
  const bool ext = a.condition != 0.0 || a.trace_norm || a.ban;
  if (a.kind == BF_MVDR) {
    if (MIX) hipLaunchKernelGGL(bf_scm<M>, g, dim3(64), 0, s, a, ws);
    else hipLaunchKernelGGL(mvdr_scm_eig<M>, g, dim3(64), 0, s, a, ws);
    const size_t lds = (size_t)a.F * M * 2 * sizeof(double);
    if (ext)
      hipLaunchKernelGGL(mvdr_solve_ext<M>, dim3(a.B, a.S), dim3(256), lds, s, a.B, a.S, a.F, (double)a.epsi, ws,
                         a.condition, a.trace_norm, a.ban);
    else
      hipLaunchKernelGGL(mvdr_solve<M>, dim3(a.B, a.S), dim3(256), lds, s, a.B, a.S, a.F, (double)a.epsi, ws);
  } else {
    if (MIX) hipLaunchKernelGGL(bf_scm<M>, g, dim3(64), 0, s, a, ws);
    else hipLaunchKernelGGL(mvdr_scm_eig<M>, g, dim3(64), 0, s, a, ws);
    if (a.kind == BF_SOUDEN)
      hipLaunchKernelGGL((bf_solve<M, BF_SOUDEN>), g, dim3(64), 0, s, a.B, a.S, a.F, (double)a.epsi, a.condition,
                         a.trace_norm, a.ban, a.bf_ref, ws);
    else
      hipLaunchKernelGGL((bf_solve<M, BF_GEV>), g, dim3(64), 0, s, a.B, a.S, a.F, (double)a.epsi, a.condition,
                         a.trace_norm, a.ban, a.bf_ref, ws);
  }
  hipLaunchKernelGGL(mvdr_apply<M>, g, dim3(256), 0, s, a, out, (const double*)ws);
  return hipGetLastError();
}

template <int M>
static hipError_t mvdr_run(const MvdrArgs& a, const COut& out, double* ws, hipStream_t s) {
  if (a.kind != BF_MVDR || a.noise_mix || a.condition != 0.0 || a.trace_norm || a.ban)
    return a.noise_mix ? bf_run<M, true>(a, out, ws, s) : bf_run<M, false>(a, out, ws, s);
  dim3 g(a.F, a.B, a.S);
  // one wave per (b, f, spk): the 6x6 Jacobi runs on one lane (~100 us of dependent float64 work), so what matters is
  // how many of them are in flight per CU -- 8 single-wave workgroups instead of 2 four-wave ones
  hipLaunchKernelGGL(mvdr_scm_eig<M>, g, dim3(64), 0, s, a, ws);
  hipLaunchKernelGGL(mvdr_solve<M>, dim3(a.B, a.S), dim3(256), (size_t)a.F * M * 2 * sizeof(double), s, a.B, a.S, a.F,
                     (double)a.epsi, ws);
  hipLaunchKernelGGL(mvdr_apply<M>, g, dim3(256), 0, s, a, out, (const double*)ws);
  return hipGetLastError();
}

hipError_t launch_mvdr(const MvdrArgs& a, const COut& out, void* ws, hipStream_t s) {
  double* w = reinterpret_cast<double*>(ws);
  switch (a.M) {
    case 2: return mvdr_run<2>(a, out, w, s);
    case 3: return mvdr_run<3>(a, out, w, s);
    case 4: return mvdr_run<4>(a, out, w, s);
    case 5: return mvdr_run<5>(a, out, w, s);
    case 6: return mvdr_run<6>(a, out, w, s);
    case 7: return mvdr_run<7>(a, out, w, s);
    case 8: return mvdr_run<8>(a, out, w, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_bf_debug(const void* ws, int B, int S, int F, int M, double* w, double* lam, hipStream_t s) {
  const double* p = reinterpret_cast<const double*>(ws);
  hipError_t e = hipSuccess;
  if (w) e = hipMemcpyAsync(w, p + ws_w(B, S, F, M), (size_t)B * S * F * M * 2 * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && lam)
    e = hipMemcpyAsync(lam, p + ws_lam(B, S, F, M), (size_t)B * S * F * sizeof(double), hipMemcpyDeviceToDevice, s);
  return e;
}

hipError_t launch_mvdr_debug(const void* ws, int B, int S, int F, int M, double* steer, double* w, hipStream_t s) {
  const double* p = reinterpret_cast<const double*>(ws);
  const size_t n = (size_t)B * S * F * M * 2 * sizeof(double);
  hipError_t e = hipSuccess;
  if (steer) e = hipMemcpyAsync(steer, p + ws_steer1(B, S, F, M), n, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && w) e = hipMemcpyAsync(w, p + ws_w(B, S, F, M), n, hipMemcpyDeviceToDevice, s);
  return e;
}

// ---- PIT distances, S speakers (1..4) -----------------------------------------------------------------------------
// part[bk][f][i][j] = sum_t | |A_i| - |B_j| | of frequency bin f   (tester.py:1047-1052, 906-908), float64.
// grid (F, B*K): blockIdx.y = b*K + k; anchors are per b, candidates per (b, k).  Every reduction runs in a fixed
// order (no atomics): pit_pick_k adds the F partials of an item in bin order, so the distances -- and with them the
// argmin over the permutations -- are bit-reproducible.
template <int S>
__global__ __launch_bounds__(256) void pit_dist_k(const PitArgs p, int K, double* part) {
  __shared__ double s_tmp[4][S * S];
  const int f = blockIdx.x, bk = blockIdx.y;
  const int b = bk / K;
  const long long oa = (long long)b * p.a.sb + (long long)f * p.a.sf;
  const long long ob = (long long)bk * p.b.sb + (long long)f * p.b.sf;
  double d[S * S];
#pragma unroll
  for (int i = 0; i < S * S; ++i) d[i] = 0.0;
  for (int t = threadIdx.x; t < p.T; t += 256) {
    const long long ia = oa + (long long)t * p.a.st, ib = ob + (long long)t * p.b.st;
    float am[S], bm[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      const float ar = p.a.re[ia + i * p.a.sm], ai = p.a.im[ia + i * p.a.sm];
      const float br = p.b.re[ib + i * p.b.sm], bi = p.b.im[ib + i * p.b.sm];
      am[i] = sqrtf(ar * ar + ai * ai);
      bm[i] = sqrtf(br * br + bi * bi);
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j < S; ++j) d[i * S + j] += fabsf(am[i] - bm[j]);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < S * S; ++i) {
    double v = d[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) s_tmp[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < S * S) {
    const int i = threadIdx.x;
    part[((long long)bk * gridDim.x + f) * (S * S) + i] = (s_tmp[0][i] + s_tmp[1][i]) + (s_tmp[2][i] + s_tmp[3][i]);
  }
}

// sel[bk][i] = perm[i] of the cheapest permutation, cost(perm) = sum_i dist[i][perm[i]]; permutations in the order of
// itertools.permutations (lexicographic), first minimum on ties (torch.argmin; tester.py:1053-1064, 909-915)
template <int S>
__global__ __launch_bounds__(64) void pit_pick_k(const double* part, int F, double* dist, int* sel) {
  __shared__ double s_d[S * S];
  const int i = blockIdx.x;                          // item (b, k)
  if (threadIdx.x < S * S) {
    const double* q = part + (long long)i * F * (S * S) + threadIdx.x;
    double acc = 0.0;
    for (int f = 0; f < F; ++f) acc += q[(long long)f * (S * S)];      // fixed order: bin 0, 1, ...
    s_d[threadIdx.x] = acc;
    dist[(long long)i * (S * S) + threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double* d = s_d;
  int perm[S], best[S];
#pragma unroll
  for (int k = 0; k < S; ++k) { perm[k] = k; best[k] = k; }
  double cbest = 0.0;
  bool first = true;
  for (;;) {
    double c = 0.0;
#pragma unroll
    for (int k = 0; k < S; ++k) c += d[k * S + perm[k]];
    if (first || c < cbest) {
      cbest = c; first = false;
#pragma unroll
      for (int k = 0; k < S; ++k) best[k] = perm[k];
    }
    // next lexicographic permutation
    int a = S - 2;
    while (a >= 0 && perm[a] > perm[a + 1]) --a;
    if (a < 0) break;
    int b2 = S - 1;
    while (perm[b2] < perm[a]) --b2;
    { const int t = perm[a]; perm[a] = perm[b2]; perm[b2] = t; }
    for (int lo = a + 1, hi = S - 1; lo < hi; ++lo, --hi) { const int t = perm[lo]; perm[lo] = perm[hi]; perm[hi] = t; }
  }
  for (int k = 0; k < S; ++k) sel[i * S + k] = best[k];
}

hipError_t launch_pit_dist_k(const PitArgs& p, int S, int K, double* part, hipStream_t s) {
  const dim3 g(p.F, p.B * K);
  switch (S) {
    case 1: hipLaunchKernelGGL(pit_dist_k<1>, g, dim3(256), 0, s, p, K, part); break;
    case 2: hipLaunchKernelGGL(pit_dist_k<2>, g, dim3(256), 0, s, p, K, part); break;
    case 3: hipLaunchKernelGGL(pit_dist_k<3>, g, dim3(256), 0, s, p, K, part); break;
    case 4: hipLaunchKernelGGL(pit_dist_k<4>, g, dim3(256), 0, s, p, K, part); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_pit_pick(const double* part, int F, int S, int n, double* dist, int* sel, hipStream_t s) {
  const dim3 g(n);
  switch (S) {
    case 1: hipLaunchKernelGGL(pit_pick_k<1>, g, dim3(64), 0, s, part, F, dist, sel); break;
    case 2: hipLaunchKernelGGL(pit_pick_k<2>, g, dim3(64), 0, s, part, F, dist, sel); break;
    case 3: hipLaunchKernelGGL(pit_pick_k<3>, g, dim3(64), 0, s, part, F, dist, sel); break;
    case 4: hipLaunchKernelGGL(pit_pick_k<4>, g, dim3(64), 0, s, part, F, dist, sel); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// final[b][m][j] = shift_sel[b][m][clean_sel[b][j]]   (tester.py:1065 then 915)
__global__ void compose_sel_k(const int* shift_sel, const int* clean_sel, int B, int M, int S, int* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * M * S) return;
  const int j = i % S, bm = i / S, b = bm / M;
  const int cj = clean_sel ? clean_sel[b * S + j] : j;
  out[i] = shift_sel[bm * S + cj];
}
hipError_t launch_compose_sel(const int* shift_sel, const int* clean_sel, int B, int M, int S, int* out,
                              hipStream_t s) {
  const int n = B * M * S;
  hipLaunchKernelGGL(compose_sel_k, dim3((n + 63) / 64), dim3(64), 0, s, shift_sel, clean_sel, B, M, S, out);
  return hipGetLastError();
}

// MISO3 input assembly (tester.py:936-939, model.py:360-364): sample n = b*S + j gets
//   channels [0,M) / [M+2, 2M+2): mixture re / im ; M / 2M+2: beamformer (written by mvdr_apply) ;
//   M+1 / 2M+3: MISO1 estimate of aligned speaker j at ref_ch.
__global__ __launch_bounds__(256) void assemble3_k(const float* in1, long long in1_bstride, const float* out1,
                                                   long long out1_bstride, const int* sel, int M, int S, int ref_ch,
                                                   int F, int Tp, float* in3, long long in3_bstride) {
  const int cch = blockIdx.x;          // 0..2M-1 mixture planes, 2M: est re, 2M+1: est im
  const int n3 = blockIdx.y;           // b*S + j
  const int b = n3 / S, j = n3 - b * S;
  const long long plane = (long long)F * Tp;
  const float* src;
  int cd3;
  if (cch < 2 * M) {
    src = in1 + (long long)(b * M) * in1_bstride + (long long)cch * plane;      // shift-0 sample = un-rolled mixture
    cd3 = cch < M ? cch : cch + 2;
  } else {
    const int n1 = b * M + ref_ch;
    const int q = sel[n1 * S + j];
    const int im = cch - 2 * M;
    src = out1 + (long long)n1 * out1_bstride + (long long)(im * S + q) * plane;
    cd3 = im ? 2 * M + 3 : M + 1;
  }
  float4* d = reinterpret_cast<float4*>(in3 + (long long)n3 * in3_bstride + (long long)cd3 * plane);
  const float4* s4 = reinterpret_cast<const float4*>(src);
  for (long long i = threadIdx.x + (long long)blockIdx.z * 256; i < plane / 4; i += 256LL * gridDim.z) d[i] = s4[i];
}
hipError_t launch_assemble3(const float* in1, long long in1_bstride, const float* out1, long long out1_bstride,
                            const int* sel, int B, int M, int S, int ref_ch, int F, int Tp, float* in3,
                            long long in3_bstride, hipStream_t s) {
  hipLaunchKernelGGL(assemble3_k, dim3(2 * M + 2, B * S, 16), dim3(256), 0, s, in1, in1_bstride, out1, out1_bstride,
                     sel, M, S, ref_ch, F, Tp, in3, in3_bstride);
  return hipGetLastError();
}

}  // namespace mn
