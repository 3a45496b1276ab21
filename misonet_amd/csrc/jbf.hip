// Joint multi-speaker beamformers on the device: LCMV (LCMP with noise "mix"), the speech-distortion-weighted multichannel Wiener
// filter and the rank-1 MWF, all S speakers of a bin solved together.  C ABI misonet_beamform_joint / misonet_beamform_joint_debug /
// misonet_pipeline_set_joint in api_array.hip and api_pipeline.hip; the definition is INTEGRATION.md 4m, restated in NumPy in
// tests/jbf_ref.py.
//
// Per (item b, bin f), independent of every other: Y = mix[b, f] [M, T], X_s the source estimate of speaker s [M, T], complex64 as
// loaded, float64 after the loads.  V = Y - sum_s X_s, Phi_s = X_s X_s^H / T, Phi_v = V V^H / T (noise "mix": Y Y^H / T),
// R = Phi_v + diag_load tr(Phi_v) / M I, N_s = sum_{j != s} Phi_j + R.
//
//   jbf_bin_k   one workgroup of 8 waves per (b, f):
//                 a sweep over the frames, SG_TT at a time through LDS (sg_stage_rows): the mixture and the S estimates as float32
//                 windows, from them the float64 frame-major rows [Re; Im] of the S + 1 classes (S speakers, then V or Y); wave k
//                 adds the tile to ITS 16 x 16 float64 MFMA accumulator, the Gram matrix of class k (sg_gram_tile1, weight 1);
//                 the covariances from the lower triangles (sg_tile1_entry), mirrored, a real diagonal; sg_diag_load;
//                 lcmv:  R = L L^H (sg_cholesky), once per bin; a_s = L q_s with q_s the principal eigenvector of
//                        C_s = L^-1 Phi_s L^-H (rtf "cw") or a_s = the principal eigenvector of Phi_s (rtf "eig"), both by
//                        jacobi_hermitian<M>; d_s = a_s / a_s[ref]; Z = L^-1 D, G = Z^H Z = K K^H, W = L^-H Z G^-1;
//                 mwf:   w_s = (Phi_s + mu N_s)^-1 Phi_s e_ref, a Cholesky and two triangular solves per speaker;
//                 r1mwf: A_s = N_s^-1 Phi_s, w_s = A_s e_ref / (mu + tr A_s) (the complex trace);
//                 a second sweep: out_s[t] = w_s^H y[t] for the S speakers from one staged mixture tile, rounded to complex64
//                 once, on the store
//
// Every sum runs in a fixed order -- the MFMA chain tile by tile in ascending t, every small sum in index order on one thread --
// nothing is accumulated with atomics and a workgroup never looks at another one: the result is bit-reproducible and depends
// neither on B nor on the position in the batch (on S it depends by definition).  Nothing is clamped.  lcmv FAILS as a whole bin
// (a pivot of R or G not finite or not > 0, a tr Phi_s that is 0 or not finite, an a_s[ref] that is 0 or not finite); mwf and
// r1mwf fail per speaker (a pivot; for r1mwf mu + tr A_s 0 or not finite): w = 0, out = 0, fail = 1.  Equal leading eigenvalues
// make d_s arbitrary; that case is NOT detected.
//
// Limits: 2 <= M <= 8 (2 M <= 16 rows: one tile), 1 <= S <= 4 (one wave per class), S <= M.  63 KB of static LDS, nothing that
// grows with T: the small matrices of the solve lie over the float64 rows, which are dead by then.
#include "kernels.hpp"
#include "cplx.hpp"
#include "stacked_gram.hpp"
#include "jacobi.hpp"

namespace mn {

constexpr int JB_CMAX = 5;            // classes: four speakers and the noise
constexpr int JB_ZP = 17;             // pitch of a frame's 16 rows, in doubles (odd)

// workspace: fail int [B][S][F] | w c128 [B][S][F][M] | (lcmv) d c128 [B][S][F][M]
struct JbWs { long long fail, w, d, total; };
__host__ __device__ inline JbWs jb_ws(int B, int S, int F, int M, int kind) {
  JbWs w;
  const long long n = (long long)B * S * F;
  w.fail = 0;
  w.w = sg_align(n * 4);
  w.d = sg_align(w.w + n * M * 16);
  w.total = kind == JBF_LCMV ? sg_align(w.d + n * M * 16) : w.d;
  return w;
}
long long jbf_ws_bytes(int B, int S, int F, int M, int kind) { return jb_ws(B, S, F, M, kind).total; }

// LDS of the solve, in bytes from the start of the float64 rows it lies over
struct JbLds {
  static constexpr int gs = 0;                              // double [C][16][16]: the Gram tiles after the sweep
  static constexpr int phi = gs + JB_CMAX * 256 * 8;        // double2 [C][M][M]: Phi_0 .. Phi_{S-1}, then R; whole Hermitian matrices
  static constexpr int rf = phi + JB_CMAX * 64 * 16;        // double2 [M][M]: L of R = L L^H (lcmv)
  static constexpr int af = rf + 64 * 16;                   // double2 [S][M][M]: the matrix factored per speaker; lcmv: C_s
  static constexpr int xs = af + 4 * 64 * 16;               // double2 [S][M][M]: A_s (r1mwf); lcmv: L^-1 Phi_s
  static constexpr int ja = xs + 4 * 64 * 16;               // double [M][M][2]: the Jacobi's matrix ...
  static constexpr int jv = ja + 64 * 16;                   // ... and its eigenvectors
  static constexpr int dm = jv + 64 * 16;                   // double2 [S][8]: a_s, then d_s
  static constexpr int zm = dm + 4 * 8 * 16;                // double2 [S][8]: Z = L^-1 D, column s
  static constexpr int um = zm + 4 * 8 * 16;                // double2 [S][8]: Z G^-1, column s
  static constexpr int wm = um + 4 * 8 * 16;                // double2 [S][8]: the weights
  static constexpr int gm = wm + 4 * 8 * 16;                // double2 [S][S]: G, then K
  static constexpr int em = gm + 16 * 16;                   // double2 [S][S]: G^-1
  static constexpr int total = em + 16 * 16;
};
static_assert(SG_TT == 64, "the row builder splits an element index into (row, frame) by 6 bits");
static_assert(JbLds::total <= JB_CMAX * SG_TT * JB_ZP * 8, "the solve must fit the rows it lies over");

// a - b c, a - conj(b) c, a + b c, a + conj(b) c, a / b
__device__ __forceinline__ double2 jb_msub(double2 a, double2 b, double2 c) {
  a.x -= b.x * c.x - b.y * c.y;
  a.y -= b.x * c.y + b.y * c.x;
  return a;
}
__device__ __forceinline__ double2 jb_msubc(double2 a, double2 b, double2 c) {
  a.x -= b.x * c.x + b.y * c.y;
  a.y -= b.x * c.y - b.y * c.x;
  return a;
}
__device__ __forceinline__ double2 jb_madd(double2 a, double2 b, double2 c) {
  a.x += b.x * c.x - b.y * c.y;
  a.y += b.x * c.y + b.y * c.x;
  return a;
}
__device__ __forceinline__ double2 jb_maddc(double2 a, double2 b, double2 c) {
  a.x += b.x * c.x + b.y * c.y;
  a.y += b.x * c.y - b.y * c.x;
  return a;
}
__device__ __forceinline__ double2 jb_div(double2 a, double2 b) {
  const double d = b.x * b.x + b.y * b.y;
  return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}

// L x = v and L^H x = v in place, L [n][n] lower (pitch n, a real diagonal), x with stride xs; one thread
__device__ __forceinline__ void jb_fwd(const double2* L, int n, double2* x, int xs) {
  for (int i = 0; i < n; ++i) {
    double2 v = x[i * xs];
    for (int k = 0; k < i; ++k) v = jb_msub(v, L[i * n + k], x[k * xs]);
    const double d = L[i * n + i].x;
    x[i * xs] = make_double2(v.x / d, v.y / d);
  }
}
__device__ __forceinline__ void jb_bwd(const double2* L, int n, double2* x, int xs) {
  for (int i = n - 1; i >= 0; --i) {
    double2 v = x[i * xs];
    for (int k = i + 1; k < n; ++k) v = jb_msubc(v, L[k * n + i], x[k * xs]);      // (L^H)[i][k] = conj(L[k][i])
    const double d = L[i * n + i].x;
    x[i * xs] = make_double2(v.x / d, v.y / d);
  }
}

template <int M>
__device__ __forceinline__ void jb_jacobi_m(double* A, double* V, int tid) {
  jacobi_hermitian<M>(*reinterpret_cast<double (*)[M][M][2]>(A), *reinterpret_cast<double (*)[M][M][2]>(V), tid);
}
// jacobi_hermitian<M> on A, V [M][M][2] for the kernel's run-time M (the same on every thread)
__device__ __forceinline__ void jb_jacobi(double* A, double* V, int M, int tid) {
  switch (M) {
    case 2: jb_jacobi_m<2>(A, V, tid); break;
    case 3: jb_jacobi_m<3>(A, V, tid); break;
    case 4: jb_jacobi_m<4>(A, V, tid); break;
    case 5: jb_jacobi_m<5>(A, V, tid); break;
    case 6: jb_jacobi_m<6>(A, V, tid); break;
    case 7: jb_jacobi_m<7>(A, V, tid); break;
    default: jb_jacobi_m<8>(A, V, tid); break;
  }
}

// grid (F, B), 512 threads
__global__ __launch_bounds__(SG_THREADS) void jbf_bin_k(const JbfArgs a, const COut out, int* fail_out, double2* w_out,
                                                        double2* d_out) {
  __shared__ float fwin[JB_CMAX * 16 * SG_TT];      // [1 + S][2 M][TT]: the staged mixture, then the S estimates
  __shared__ __align__(16) double rows[JB_CMAX * SG_TT * JB_ZP];   // [C][TT][16 (+ 1)]: [Re; Im] of a frame per class; then JbLds
  __shared__ double ones[SG_TT];
  __shared__ double2 col[8];
  __shared__ double red[SG_WAVES];
  __shared__ int sbad[4];
  const int M = a.M, T = a.T, S = a.S, NC = S + 1;
  const int f = blockIdx.x, b = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;
  unsigned char* sol = reinterpret_cast<unsigned char*>(rows);
  double* gs = reinterpret_cast<double*>(sol + JbLds::gs);
  double2* Phi = reinterpret_cast<double2*>(sol + JbLds::phi);
  double2* Rf = reinterpret_cast<double2*>(sol + JbLds::rf);
  double2* Af = reinterpret_cast<double2*>(sol + JbLds::af);
  double2* Xs = reinterpret_cast<double2*>(sol + JbLds::xs);
  double2* jA = reinterpret_cast<double2*>(sol + JbLds::ja);
  double2* jV = reinterpret_cast<double2*>(sol + JbLds::jv);
  double2* Dm = reinterpret_cast<double2*>(sol + JbLds::dm);
  double2* Zm = reinterpret_cast<double2*>(sol + JbLds::zm);
  double2* Um = reinterpret_cast<double2*>(sol + JbLds::um);
  double2* Wm = reinterpret_cast<double2*>(sol + JbLds::wm);
  double2* Gm = reinterpret_cast<double2*>(sol + JbLds::gm);
  double2* Em = reinterpret_cast<double2*>(sol + JbLds::em);
  const long long yoff = (long long)b * a.mix.sb + (long long)f * a.mix.sf;
  const float* yre = a.mix.re + yoff;
  const float* yim = a.mix.im + yoff;
  const long long yst = a.mix.st;
  const auto load_y = [&](int m, int t) {
    return make_float2(yre[(long long)m * a.mix.sm + t * yst], yim[(long long)m * a.mix.sm + t * yst]);
  };
  const int ntile_t = (T + SG_TT - 1) / SG_TT;
  const int MM = M * M;

  if (tid < SG_TT) ones[tid] = 1.0;

  // ---- the Gram matrices of the S + 1 classes, class k on wave k
  d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * SG_TT;
    __syncthreads();                                                   // the tile before is consumed
    sg_stage_rows(load_y, M, T, t0, fwin);
    for (int s = 0; s < S; ++s) {
      const auto load_s = [&](int m, int t) {
        const float *sre, *sim;
        int sst;
        src_row(a, b, f, m, s, sre, sim, sst);
        const long long o = (a.est ? 0 : (long long)s * a.src_ss) + (long long)t * sst;
        return make_float2(sre[o], sim[o]);
      };
      sg_stage_rows(load_s, M, T, t0, fwin + (1 + s) * 16 * SG_TT);
    }
    __syncthreads();
    // the float64 rows: class s = X_s, class S = V = Y - sum_s X_s (or Y); the frames past T are staged as zeros
    for (int e = tid; e < 16 * SG_TT; e += SG_THREADS) {
      const int r = e >> 6, tl = e & (SG_TT - 1);
      const bool in = r < 2 * M;
      double sum = 0.0;
      for (int s = 0; s < S; ++s) {                                    // fixed order: speaker 0, 1, ...
        const double x = in ? (double)fwin[(1 + s) * 16 * SG_TT + r * SG_TT + tl] : 0.0;
        rows[(s * SG_TT + tl) * JB_ZP + r] = x;
        sum += x;
      }
      const double y = in ? (double)fwin[r * SG_TT + tl] : 0.0;
      rows[(S * SG_TT + tl) * JB_ZP + r] = a.noise_mix ? y : y - sum;
    }
    __syncthreads();
    if (wave < NC) sg_gram_tile1(acc, rows + wave * SG_TT * JB_ZP, JB_ZP, ones);
  }
  __syncthreads();                                                     // the rows are dead: the solve lies over them

  // ---- the covariances: the lower triangle from the tile, mirrored, a real diagonal
  if (wave < NC) {
#pragma unroll
    for (int r = 0; r < 4; ++r) gs[wave * 256 + (lg + 4 * r) * 16 + lr] = acc[r];
  }
  if (tid < 4) sbad[tid] = 0;
  __syncthreads();
  for (int e = tid; e < NC * MM; e += SG_THREADS) {
    const int c = e / MM, r = e - c * MM, i = r / M, j = r - i * M;
    const int hi = i >= j ? i : j, lo = i >= j ? j : i;
    double2 v = sg_tile1_entry(gs + c * 256, M, hi, lo);
    v.x /= (double)T;
    v.y /= (double)T;
    if (i < j) v.y = -v.y;
    Phi[c * 64 + r] = v;
  }
  __syncthreads();
  double2* R = Phi + S * 64;
  if (a.diag_load != 0.0) {
    sg_diag_load(R, M, a.diag_load, red);
    __syncthreads();
  }

  // failed: bit s = speaker s has no solution (every condition below is the same on every thread)
  unsigned failed = 0;
  const unsigned all = (1u << S) - 1u;
  if (a.kind == JBF_LCMV) {
    for (int e = tid; e < MM; e += SG_THREADS) Rf[e] = R[e];
    __syncthreads();
    if (!sg_cholesky(Rf, M, M, col)) failed = all;
    for (int s = 0; s < S && !failed; ++s) {                           // an exactly-zero estimate has no direction
      double tr = 0.0;
      for (int i = 0; i < M; ++i) tr += Phi[s * 64 + i * M + i].x;
      if (tr == 0.0 || !finite(tr)) failed = all;
    }
    if (!failed) {
#pragma unroll 1
      for (int s = 0; s < S; ++s) {
        const double2* Ps = Phi + s * 64;
        double2* X = Xs + s * 64;
        double2* Cs = Af + s * 64;
        __syncthreads();                                               // the Jacobi of the speaker before is read
        if (!a.rtf_eig) {
          for (int e = tid; e < MM; e += SG_THREADS) X[e] = Ps[e];
          __syncthreads();
          if (tid < M) jb_fwd(Rf, M, X + tid, M);                      // X = L^-1 Phi_s, column tid
          __syncthreads();
          if (tid < M) {                                               // row tid of C = X L^-H: L c = conj(X[tid, :])^T, C[tid][i] = conj(c_i)
            double2* c = Cs + tid * M;
            for (int i = 0; i < M; ++i) c[i] = make_double2(X[tid * M + i].x, -X[tid * M + i].y);
            jb_fwd(Rf, M, c, 1);
            for (int i = 0; i < M; ++i) c[i].y = -c[i].y;
          }
          __syncthreads();
        }
        for (int e = tid; e < MM; e += SG_THREADS) {
          const int i = e / M, j = e - i * M;
          double2 v = Ps[e];
          if (!a.rtf_eig) {                                            // the Hermitian part of C (it is Hermitian up to rounding)
            const double2 cij = Cs[i * M + j], cji = Cs[j * M + i];
            v = make_double2(0.5 * (cij.x + cji.x), i == j ? 0.0 : 0.5 * (cij.y - cji.y));
          }
          jA[e] = v;
          jV[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
        }
        __syncthreads();
        jb_jacobi(reinterpret_cast<double*>(jA), reinterpret_cast<double*>(jV), M, tid);
        int best = 0;                                                  // largest eigenvalue, first on ties
        for (int i = 1; i < M; ++i)
          if (jA[i * M + i].x > jA[best * M + best].x) best = i;
        if (tid < M) {                                                 // a = L q (cw) or q (eig)
          double2 v = jV[tid * M + best];
          if (!a.rtf_eig) {
            v = make_double2(0.0, 0.0);
            for (int k = 0; k <= tid; ++k) v = jb_madd(v, Rf[tid * M + k], jV[k * M + best]);
          }
          Dm[s * 8 + tid] = v;
        }
      }
      __syncthreads();
      // d_s = a_s / a_s[ref]
      double2 aref = make_double2(1.0, 0.0);
      for (int s = 0; s < S; ++s) {
        const double2 v = Dm[s * 8 + a.ref];
        if ((v.x == 0.0 && v.y == 0.0) || !finite(v.x) || !finite(v.y)) failed = all;
        if (tid / M == s) aref = v;
      }
      __syncthreads();
      if (!failed && tid < S * M) {
        const int s = tid / M, i = tid - s * M;
        const double2 d = i == a.ref ? make_double2(1.0, 0.0) : jb_div(Dm[s * 8 + i], aref);
        Dm[s * 8 + i] = d;
        Zm[s * 8 + i] = d;
      }
      __syncthreads();
    }
    if (!failed) {
      if (tid < S) jb_fwd(Rf, M, Zm + tid * 8, 1);                     // Z = L^-1 D, column tid
      __syncthreads();
      if (tid < S * S) {                                               // G = Z^H Z, the lower triangle
        const int i = tid / S, j = tid - i * S;
        if (i >= j) {
          double2 v = make_double2(0.0, 0.0);
          for (int m = 0; m < M; ++m) v = jb_maddc(v, Zm[i * 8 + m], Zm[j * 8 + m]);
          if (i == j) v.y = 0.0;
          Gm[i * S + j] = v;
        }
      }
      __syncthreads();
      if (!sg_cholesky(Gm, S, S, col)) failed = all;
    }
    if (!failed) {
      __syncthreads();
      if (tid < S) {                                                   // column tid of G^-1
        for (int i = 0; i < S; ++i) Em[i * S + tid] = make_double2(i == tid ? 1.0 : 0.0, 0.0);
        jb_fwd(Gm, S, Em + tid, S);
        jb_bwd(Gm, S, Em + tid, S);
      }
      __syncthreads();
      if (tid < S * M) {                                               // U = Z G^-1
        const int s = tid / M, m = tid - s * M;
        double2 v = make_double2(0.0, 0.0);
        for (int j = 0; j < S; ++j) v = jb_madd(v, Zm[j * 8 + m], Em[j * S + s]);
        Um[s * 8 + m] = v;
      }
      __syncthreads();
      if (tid < S) {                                                   // w_s = L^-H u_s
        jb_bwd(Rf, M, Um + tid * 8, 1);
        for (int m = 0; m < M; ++m) Wm[tid * 8 + m] = Um[tid * 8 + m];
      }
    }
  } else {
    const bool mwf = a.kind == JBF_MWF;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      double2* A = Af + s * 64;
      for (int e = tid; e < MM; e += SG_THREADS) {                     // N_s = sum_{j != s} Phi_j + R, fixed order: j = 0, 1, ...
        double2 n = make_double2(0.0, 0.0);
        for (int j = 0; j < S; ++j)
          if (j != s) { n.x += Phi[j * 64 + e].x; n.y += Phi[j * 64 + e].y; }
        n.x += R[e].x;
        n.y += R[e].y;
        A[e] = mwf ? make_double2(Phi[s * 64 + e].x + a.mu * n.x, Phi[s * 64 + e].y + a.mu * n.y) : n;
      }
      __syncthreads();
      if (!sg_cholesky(A, M, M, col)) failed |= 1u << s;
      __syncthreads();
    }
    if (mwf) {
      if (tid < S && !((failed >> tid) & 1u)) {                        // w_s = A^-1 Phi_s e_ref
        for (int i = 0; i < M; ++i) Wm[tid * 8 + i] = Phi[tid * 64 + i * M + a.ref];
        jb_fwd(Af + tid * 64, M, Wm + tid * 8, 1);
        jb_bwd(Af + tid * 64, M, Wm + tid * 8, 1);
      }
    } else {
      if (tid < S * M) {                                               // A_s = N_s^-1 Phi_s, column j
        const int s = tid / M, j = tid - s * M;
        if (!((failed >> s) & 1u)) {
          for (int i = 0; i < M; ++i) Xs[s * 64 + i * M + j] = Phi[s * 64 + i * M + j];
          jb_fwd(Af + s * 64, M, Xs + s * 64 + j, M);
          jb_bwd(Af + s * 64, M, Xs + s * 64 + j, M);
        }
      }
      __syncthreads();
      if (tid < S && !((failed >> tid) & 1u)) {                        // w_s = A_s e_ref / (mu + tr A_s)
        double2 den = make_double2(a.mu, 0.0);
        for (int i = 0; i < M; ++i) { den.x += Xs[tid * 64 + i * M + i].x; den.y += Xs[tid * 64 + i * M + i].y; }
        if ((den.x == 0.0 && den.y == 0.0) || !finite(den.x) || !finite(den.y)) sbad[tid] = 1;
        else
          for (int i = 0; i < M; ++i) Wm[tid * 8 + i] = jb_div(Xs[tid * 64 + i * M + a.ref], den);
      }
      __syncthreads();
      for (int s = 0; s < S; ++s)
        if (sbad[s]) failed |= 1u << s;
    }
  }
  __syncthreads();
  if (tid < S * M) {                                                   // a failed speaker: w = 0 (and d = 0)
    const int s = tid / M, m = tid - s * M;
    const bool bad = (failed >> s) & 1u;
    if (bad) Wm[s * 8 + m] = make_double2(0.0, 0.0);
    const long long o = (((long long)b * S + s) * a.F + f) * M + m;
    w_out[o] = Wm[s * 8 + m];
    if (a.kind == JBF_LCMV) d_out[o] = bad ? make_double2(0.0, 0.0) : Dm[s * 8 + m];
  }
  if (tid < S) fail_out[((long long)b * S + tid) * a.F + f] = (failed >> tid) & 1u;

  // ---- out_s[t] = w_s^H y[t]: speaker s on wave s, a frame per lane; microphone 0, 1, ... in turn
#pragma unroll 1
  for (int tt = 0; tt < ntile_t; ++tt) {
    const int t0 = tt * SG_TT, t = t0 + lane;
    __syncthreads();
    sg_stage_rows(load_y, M, T, t0, fwin);
    __syncthreads();
    if (wave < S && t < T) {
      double sr = 0.0, si = 0.0;
      for (int m = 0; m < M; ++m) {
        const double2 w = Wm[wave * 8 + m];
        const double vr = (double)fwin[m * SG_TT + lane], vi = (double)fwin[(M + m) * SG_TT + lane];
        sr += w.x * vr + w.y * vi;                                     // conj(w) y
        si += w.x * vi - w.y * vr;
      }
      const bool bad = (failed >> wave) & 1u;
      const long long o = (long long)b * out.ob + (long long)wave * out.os + (long long)f * out.of + (long long)t * out.ot;
      out.re[o] = bad ? 0.f : (float)sr;
      out.im[o] = bad ? 0.f : (float)si;
    }
  }
}

hipError_t launch_jbf(const JbfArgs& a, const COut& out, void* ws, hipStream_t s) {
  if (a.M < 2 || a.M > 8 || a.S < 1 || a.S > 4 || a.S > a.M || a.T < 1 || a.B < 1 || a.B > 65535 || a.F < 1 || a.ref < 0 ||
      a.ref >= a.M || a.kind < JBF_LCMV || a.kind > JBF_R1MWF)
    return hipErrorInvalidValue;
  const JbWs w = jb_ws(a.B, a.S, a.F, a.M, a.kind);
  char* base = reinterpret_cast<char*>(ws);
  hipLaunchKernelGGL(jbf_bin_k, dim3(a.F, a.B), dim3(SG_THREADS), 0, s, a, out, reinterpret_cast<int*>(base + w.fail),
                     reinterpret_cast<double2*>(base + w.w), reinterpret_cast<double2*>(base + w.d));
  return hipGetLastError();
}

hipError_t launch_jbf_debug(const void* ws, int B, int S, int F, int M, int kind, void* w, void* d, int* fail, hipStream_t s) {
  const JbWs l = jb_ws(B, S, F, M, kind);
  const char* base = reinterpret_cast<const char*>(ws);
  const long long n = (long long)B * S * F;
  hipError_t e = hipSuccess;
  if (w) e = hipMemcpyAsync(w, base + l.w, n * M * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && d) e = hipMemcpyAsync(d, base + l.d, n * M * 16, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess && fail) e = hipMemcpyAsync(fail, base + l.fail, n * 4, hipMemcpyDeviceToDevice, s);
  return e;
}

}  // namespace mn
