// Online AuxIVA for fewer sources than microphones (OverIVA; Scheibler & Ono 2019, in the frame-recursive form of oiva.hip) on
// the device: C ABI misonet_overiva* in api_array.hip; the definition is INTEGRATION.md 4w and is restated in NumPy in
// tests/overiva_ref.py.  The project's own definition; nothing was compared against pyroomacoustics or torchiva.
//
// K sources at M microphones, 1 <= K <= M - 1.  The state of (item b, bin f) is Ws [K][M] (row k = w_k^H, y = Ws x), J [M - K][K],
// V [K][M][M] (one Hermitian matrix per source) and C [M][M] (Hermitian, the recursive mixture covariance), complex128, the
// frame count n and the fail word.  The full demixing matrix is W = [Ws ; J, -I].  Per new frame, float64 after the load:
//
//   0. a bin whose frame holds a non-finite sample: fail |= 1, x = 0 below, step 3 skipped, its outputs 0
//   1. yt_k[f] = sum_m Ws_f[k][m] x_f[m]                     Ws as it stood before the frame
//   2. r_k = sum_f |yt_k[f]|^2,  phi_k = 1 / max(r_k / F, floor) (gauss) or 1 / max(2 sqrt(r_k), floor) (laplace)
//   3. per bin:  C <- alpha C + (1 - alpha) x x^H, then for k = 0 .. K - 1:
//        V_k <- alpha V_k + (1 - alpha) phi_k x x^H,  (W V_k) u = e_k with the full W as it stands,  d = Re(u^H V_k u),
//        row k of Ws <- conj(u) / sqrt(d); a pivot 0 or non-finite, d not finite or not > 0: the row stays, fail |= 2
//        J re-solved after every k: P = C Ws^H [M][K], J P1 = P2 as P1^T J^T = P2^T (K x K, M - K right-hand sides); a pivot 0
//        or non-finite: J stays, fail |= 8
//   4. y = Ws x, S = Ws[:, :K] + Ws[:, K:] J, A_top = S^-1, A_bot = J A_top, est[k] = A[ref][k] y_k, images[k][m] = A[m][k] y_k;
//      S singular: fail |= 4, outputs 0
//   5. n <- n + 1 (it stops at 2^31 - 1)
//
//   overiva_reset_k   every 16 bytes of the state: Ws = [I 0], J = 0, V_k = init I, C = init I, the rest 0
//   overiva_k<M, K>   the plan of oiva_k<M>, for its reason (step 2 couples all bins of an item once per frame): one workgroup per
//                     item walks the T frames of the call in order, two barriers per frame, no workgroup ever waits for another.
//                     A group of G = lanes_for(M) lanes owns a bin; lane j holds row j of the full W -- a row of Ws for j < K,
//                     [J[j - K, :], -e_j] beyond -- so the M x M elimination is oiva_solve as oiva_k uses it.  The state goes
//                     through global memory in every frame (M = 6, K = 2, F = 129: under 0.4 MB, it stays in L2); the LDS holds
//                     |yt|^2 [K][F] and phi only.
//                       - C and V_k: every lane of the group forms the whole updated matrix from the stored lower triangle (the
//                         same instructions on the same operands: the same bits on every lane), the upper triangle is its
//                         conjugate and the diagonal's imaginary part is 0, so the stored matrices are exactly Hermitian.  C is
//                         formed anew from the stored one for every k and written back behind the last.
//                       - J: row i of P1^T | P2^T is sum_m C[r][m] conj(Ws[i][m]) over r: lane i < K forms it from its own row of
//                         Ws as C comes by; oiva_solve<K, G, M - K> solves, lane K + r keeps row r of J as the solution comes by.
//
// Every sum has one fixed order that depends on M, K and F only and nothing is accumulated with atomics: the result is
// bit-reproducible, does not depend on the batch or the position in it, and does not depend on how the stream is cut into calls.
// One launch, no host synchronisation, no allocation; nothing in the launch or the state depends on T.
#include "kernels.hpp"
#include "cplx.hpp"
#include "oiva_solve.hpp"

namespace mn {

constexpr int OVERIVA_FMAX = 1025;

template <int M, int K> struct OverivaGeom {
  static constexpr int G = lanes_for(M);                               // lanes per bin
  // the registers of a lane are those of the rows of W, W V_k, V_k and u, as in oiva_k<M>: they grow with M, hardly with K
  static constexpr int THREADS = M <= 2 ? 1024 : M <= 3 ? 768 : M <= 5 ? 512 : 256;
  static constexpr int BINS = THREADS / G;                             // bins per pass
};

// host: f(integral_constant<M>, integral_constant<K>) for 2 <= M <= 8, 1 <= K <= M - 1: the caller checks the range
template <class F> static void with_mk(int M, int K, F&& f) {
  with_m(M, [&](auto m) {
    constexpr int Mc = decltype(m)::value;
    auto go = [&](auto k) {
      if constexpr (decltype(k)::value < Mc) f(m, k);
    };
    switch (K) {
      case 1: go(std::integral_constant<int, 1>{}); break;
      case 2: go(std::integral_constant<int, 2>{}); break;
      case 3: go(std::integral_constant<int, 3>{}); break;
      case 4: go(std::integral_constant<int, 4>{}); break;
      case 5: go(std::integral_constant<int, 5>{}); break;
      case 6: go(std::integral_constant<int, 6>{}); break;
      default: go(std::integral_constant<int, 7>{}); break;
    }
  });
}

int overiva_bins_per_pass(int M, int K) {
  int bins = -1;
  if (M >= 2 && M <= 8 && K >= 1 && K < M)
    with_mk(M, K, [&](auto m, auto k) { bins = OverivaGeom<decltype(m)::value, decltype(k)::value>::BINS; });
  return bins;
}

// state: fail int [bins] | n int [bins] | Ws c128 [bins][K][M] | J c128 [bins][M - K][K] | V c128 [bins][K][M][M] | C c128 [bins][M][M]
struct OverivaWs { long long fail, n, W, J, V, C, total; };
__host__ __device__ inline OverivaWs overiva_ws(long long bins, int M, int K) {
  OverivaWs w;
  w.fail = 0;
  w.n = align16(bins * 4);
  w.W = align16(w.n + bins * 4);
  w.J = w.W + bins * K * M * 16;
  w.V = w.J + bins * (M - K) * K * 16;
  w.C = w.V + bins * K * M * M * 16;
  w.total = w.C + bins * M * M * 16;
  return w;
}
long long overiva_state_bytes(long long bins, int M, int K) { return overiva_ws(bins, M, K).total; }

struct OverivaArgs {
  const float2* mix;
  float2 *est, *img;
  char* state;
  OverivaWs w;
  int T, F, model, ref;
  double alpha, oma, floor;                                            // oma = 1 - alpha
};

// grid (ceil(total / 16 / 256)), 256 threads: every 16 bytes of the state
__global__ __launch_bounds__(256) void overiva_reset_k(char* state, long long bins, int M, int K, double init) {
  const OverivaWs w = overiva_ws(bins, M, K);
  const long long units = w.total / 16, nw = bins * K * M, nv = nw * M, nc = bins * M * M;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
    const long long off = u * 16;
    double2 v = make_double2(0.0, 0.0);
    if (off >= w.C) {
      const long long e = (off - w.C) / 16;
      if (e < nc && (e / M) % M == e % M) v.x = init;
    } else if (off >= w.V) {
      const long long e = (off - w.V) / 16;
      if (e < nv && (e / M) % M == e % M) v.x = init;
    } else if (off >= w.J) {
    } else if (off >= w.W) {
      const long long e = (off - w.W) / 16;
      if (e < nw && (e / M) % K == e % M) v.x = 1.0;
    }
    *reinterpret_cast<double2*>(state + off) = v;
  }
}

// a value the compiler knows nothing about: a test on it is made where it stands and its mask is not kept in SGPRs from there on
__device__ __forceinline__ int overiva_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// grid (B), OverivaGeom<M, K>::THREADS threads
template <int M, int K>
__global__ __launch_bounds__((OverivaGeom<M, K>::THREADS)) void overiva_k(const OverivaArgs a) {
  using Geom = OverivaGeom<M, K>;
  constexpr int G = Geom::G, THREADS = Geom::THREADS, BINS = Geom::BINS, R = M - K;
  __shared__ double part[K * OVERIVA_FMAX];                            // |yt_k[f]|^2 at [k][f]
  __shared__ double phil[8];

  const int T = a.T, F = a.F;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = tid & (G - 1), slot = tid / G;
  // a run-time index into a register array is a chain of tests on one opaque bit each (oiva_k has the reason)
  unsigned rbit = 1u << a.ref;
  asm volatile("" : "+s"(rbit));
  const int jr = j < M ? j : M - 1;                                      // the row an idle lane of the group reads (and never writes)
  const long long bin0 = (long long)b * F, TF = (long long)T * F;
  int* failp = reinterpret_cast<int*>(a.state + a.w.fail) + bin0;
  int* np = reinterpret_cast<int*>(a.state + a.w.n) + bin0;
  double2* Wg = reinterpret_cast<double2*>(a.state + a.w.W) + bin0 * K * M;
  double2* Jg = reinterpret_cast<double2*>(a.state + a.w.J) + bin0 * R * K;
  double2* Vg = reinterpret_cast<double2*>(a.state + a.w.V) + bin0 * K * M * M;
  double2* Cg = reinterpret_cast<double2*>(a.state + a.w.C) + bin0 * M * M;
  const float2* xb = a.mix + (long long)b * M * TF;                    // frame t of microphone m: xb[(m T + t) F + f]
  float2* eb = a.est + (long long)b * K * TF;
  float2* ib = a.img ? a.img + (long long)b * K * M * TF : nullptr;
  const double alpha = a.alpha, oma = a.oma;
  if constexpr (M >= 7) {
    // from 7 microphones on the kernel is short of SGPRs and has VGPRs (AGPRs) to spare: the bases of the state's parts and of
    // the outputs are held there
    asm volatile("" : "+v"(Jg), "+v"(Vg), "+v"(Cg), "+v"(eb), "+v"(ib), "+v"(failp), "+v"(np));
  }

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    // ---- 1. |yt|^2 of every bin with Ws as it stands
#pragma unroll 1
    for (int f0 = 0; f0 < F; f0 += BINS) {
      const int f = f0 + slot;
      const bool act = f < F;
      const int fc = act ? f : F - 1;
      float2 x[M];
      oiva_load<M>(xb + (long long)t * F + fc, TF, x);
      const double2* wr = Wg + ((long long)fc * K + (j < K ? j : K - 1)) * M;
      double2 y = make_double2(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) y = c_fma(y, wr[m], c_wide(x[m]));
      if (act && j < K) part[j * OVERIVA_FMAX + f] = y.x * y.x + y.y * y.y;
    }
    __syncthreads();

    // ---- 2. r_k over the bins in one fixed order, phi_k
    for (int k = wave; k < K; k += THREADS / 64) {
      double s = 0.0;
      for (int f = lane; f < F; f += 64) s += part[k * OVERIVA_FMAX + f];
#pragma unroll
      for (int q = 32; q >= 1; q >>= 1) s += __shfl_xor(s, q, 64);
      if (lane == 0) phil[k] = 1.0 / fmax(a.model == 0 ? s / (double)F : 2.0 * sqrt(s), a.floor);
    }
    __syncthreads();

    // ---- 3 - 5. per bin: the covariances, the rows of Ws, J, the outputs
#pragma unroll 1
    for (int f0 = 0; f0 < F; f0 += BINS) {
      const int f = f0 + slot;
      const bool act = f < F;
      const int fc = act ? f : F - 1;
      float2 x[M];
      double2 Wr[M];                                                   // row j of W = [Ws ; J, -I]
      const bool bad = oiva_load<M>(xb + (long long)t * F + fc, TF, x);
      // row jr of W: M entries of Ws, or K entries of J and then -e_jr
      double2* wr = jr < K ? Wg + ((long long)fc * K + jr) * M : Jg + ((long long)fc * R + (jr - K)) * K;
#pragma unroll
      for (int m = 0; m < K; ++m) Wr[m] = wr[m];
#pragma unroll
      for (int m = K; m < M; ++m) {
        const double2 w = wr[jr < K ? m : 0];
        Wr[m] = jr < K ? w : make_double2(jr == m ? -1.0 : 0.0, 0.0);
      }
      // bit 0: the bin exists, bit 1: its frame is bad.  Kept in a VGPR and tested anew at every use (3 = 1: update and store)
      const int lv = overiva_opaque((act ? 1 : 0) | (bad ? 2 : 0));
      int flags = 0;
      int kn = K;                                                      // opaque: K = 1 keeps the shape of the loop, and its registers
      asm volatile("" : "+s"(kn));
      const double2* cg = Cg + (long long)fc * M * M;

#pragma unroll 1
      for (int k = 0; k < kn; ++k) {
        // the lane's row number, opaque and made anew in every round (oiva_k has the reason)
        int jk = j;
        asm volatile("" : "+v"(jk));
        const unsigned jbit = 1u << jk;
        {
          const double g = oma * phil[k];
          double2* vk = Vg + ((long long)fc * K + k) * M * M;
          double2 Tr[M], Vr[M];                                        // row j of W V_k and of V_k
#pragma unroll
          for (int c = 0; c < M; ++c) { Tr[c] = make_double2(0.0, 0.0); Vr[c] = Tr[c]; }
#pragma unroll
          for (int m = 0; m < M; ++m) {
#pragma unroll
            for (int c = 0; c <= m; ++c) {                             // the lower triangle; the upper is its conjugate
              const double2 o = vk[m * M + c], xm = c_wide(x[m]), xc = c_wide(x[c]);
              double2 v;
              v.x = alpha * o.x + g * (xm.x * xc.x + xm.y * xc.y);
              v.y = c == m ? 0.0 : alpha * o.y + g * (xm.y * xc.x - xm.x * xc.y);
              Tr[c] = c_fma(Tr[c], Wr[m], v);
              if (jk == m) Vr[c] = v;
              if (c < m) {
                const double2 vc = make_double2(v.x, -v.y);
                Tr[m] = c_fma(Tr[m], Wr[c], vc);
                if (jk == c) Vr[m] = vc;
              }
            }
            __builtin_amdgcn_sched_barrier(0);                         // one row at a time: the loads of all rows at once spill
          }
          if ((overiva_opaque(lv) & 3) == 1 && jk < M) {
            double2* vrow = vk + j * M;
#pragma unroll
            for (int c = 0; c < M; ++c) vrow[c] = Vr[c];
          }
          double2 rhs[1] = {make_double2(jk == k ? 1.0 : 0.0, 0.0)};
          double2 u[M];
          const bool sbad = oiva_solve<M, G, 1>(Tr, rhs, jk, [&](int c, int, double2 v) __attribute__((always_inline)) { u[c] = v; });
          double2 q = make_double2(0.0, 0.0), uj = u[0];
#pragma unroll
          for (int c = 0; c < M; ++c) {
            q = c_fma(q, Vr[c], u[c]);
            if (jbit >> c & 1u) uj = u[c];
          }
          double d = jk < M ? uj.x * q.x + uj.y * q.y : 0.0;
#pragma unroll
          for (int s = 1; s < G; s <<= 1) d += __shfl_xor(d, s, G);    // the same bits on every lane of the group
          const bool ok = !sbad && d > 0.0 && d <= F64_MAX;
          if (!ok) flags |= 2;
          if (ok && jk == k) {
            const double inv = 1.0 / sqrt(d);
#pragma unroll
            for (int c = 0; c < M; ++c) Wr[c] = make_double2(u[c].x * inv, -u[c].y * inv);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        {
          // J anew: C as updated, formed from the stored one (it is written back behind the last k); lane i < K gathers row i of
          // P1^T | P2^T, P[r] = sum_m C[r][m] conj(Ws[i][m]), m ascending
          int jq = j;
          asm volatile("" : "+v"(jq));
          const unsigned qbit = 1u << jq;
          double2 P[M], Cr[M];
#pragma unroll
          for (int c = 0; c < M; ++c) { P[c] = make_double2(0.0, 0.0); Cr[c] = P[c]; }
#pragma unroll
          for (int m = 0; m < M; ++m) {
#pragma unroll
            for (int c = 0; c <= m; ++c) {
              const double2 o = cg[m * M + c], xm = c_wide(x[m]), xc = c_wide(x[c]);
              double2 v;
              v.x = alpha * o.x + oma * (xm.x * xc.x + xm.y * xc.y);
              v.y = c == m ? 0.0 : alpha * o.y + oma * (xm.y * xc.x - xm.x * xc.y);
              P[m] = c_fma(P[m], v, make_double2(Wr[c].x, -Wr[c].y));
              if (jq == m) Cr[c] = v;
              if (c < m) {
                const double2 vc = make_double2(v.x, -v.y);
                P[c] = c_fma(P[c], vc, make_double2(Wr[m].x, -Wr[m].y));
                if (jq == c) Cr[m] = vc;
              }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if ((overiva_opaque(lv) & 3) == 1 && jq < M && k == K - 1) {
            double2* crow = Cg + (long long)fc * M * M + j * M;
#pragma unroll
            for (int c = 0; c < M; ++c) crow[c] = Cr[c];
          }
          double2 PA[K], PB[R], Jn[K];
#pragma unroll
          for (int c = 0; c < K; ++c) { PA[c] = P[c]; Jn[c] = Wr[c]; }
#pragma unroll
          for (int r = 0; r < R; ++r) PB[r] = P[K + r];
          // entry (c, r) of the solution J^T is J[r][c]: lane K + r keeps it
          const bool jbad = oiva_solve<K, G, R>(PA, PB, jq, [&](int c, int r, double2 v) __attribute__((always_inline)) {
            if (qbit >> (K + r) & 1u) Jn[c] = v;
          });
          if (jbad) flags |= 8;
          if (!jbad && jq >= K) {
#pragma unroll
            for (int c = 0; c < K; ++c) Wr[c] = Jn[c];
          }
        }
      }
      if ((overiva_opaque(lv) & 3) == 1 && overiva_opaque(j) < M) {
#pragma unroll
        for (int c = 0; c < K; ++c) wr[c] = Wr[c];
        if (overiva_opaque(j) < K) {
#pragma unroll
          for (int c = K; c < M; ++c) wr[c] = Wr[c];
        }
      }

      // ---- 4. y = Ws x, S = Ws[:, :K] + Ws[:, K:] J, A_top = S^-1, A_bot = J A_top: lane k takes column k of A
      double2 y = make_double2(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) y = c_fma(y, Wr[m], c_wide(x[m]));
      double2 Sr[K], eye[K], acol[M];
      int ja = j;
      asm volatile("" : "+v"(ja));
      const unsigned jbit = 1u << ja;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        double2 s = make_double2(0.0, 0.0);
#pragma unroll
        for (int r = 0; r < R; ++r) s = c_fma(s, Wr[K + r], c_from<G>(Wr[c], K + r));
        Sr[c] = make_double2(Wr[c].x + s.x, Wr[c].y + s.y);
        eye[c] = make_double2(c == ja ? 1.0 : 0.0, 0.0);
      }
      const bool abad = oiva_solve<K, G, K>(Sr, eye, ja, [&](int c, int r, double2 v) __attribute__((always_inline)) {
        if (r == 0 || (jbit >> r & 1u)) acol[c] = v;
      });
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double2 s = make_double2(0.0, 0.0);
#pragma unroll
        for (int c = 0; c < K; ++c) s = c_fma(s, c_from<G>(Wr[c], K + r), acol[c]);
        acol[K + r] = s;
      }
      if (abad) flags |= 4;
      const int lo = overiva_opaque(lv);
      const bool zero = (lo & 2) || abad;
      if ((lo & 1) && ja < K) {
        double2 ar = acol[0];
#pragma unroll
        for (int c = 1; c < M; ++c)
          if (rbit >> c & 1u) ar = acol[c];
        const double2 e = c_mul(ar, y);
        const long long o = (long long)t * F + f;
        eb[j * TF + o] = zero ? make_float2(0.f, 0.f) : make_float2((float)e.x, (float)e.y);
        if (ib) {
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const double2 v = c_mul(acol[m], y);
            ib[((long long)j * M + m) * TF + o] = zero ? make_float2(0.f, 0.f) : make_float2((float)v.x, (float)v.y);
          }
        }
      }
      // ---- 5. the flags and the frame count of the bin
      if ((lo & 1) && ja == 0) {
        if (lo & 2) flags = 1;                                         // a bad frame: that flag and no other
        if (flags) failp[f] |= flags;
        const int n = np[f];
        if (n < 0x7fffffff) np[f] = n + 1;
      }
    }
  }
}

hipError_t launch_overiva_reset(void* state, int B, int M, int K, int F, double init, hipStream_t s) {
  const long long bins = (long long)B * F, units = overiva_state_bytes(bins, M, K) / 16;
  const long long blocks = (units + 255) / 256;
  hipLaunchKernelGGL(overiva_reset_k, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s,
                     reinterpret_cast<char*>(state), bins, M, K, init);
  return hipGetLastError();
}

template <int M, int K> static void overiva_go(const OverivaArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL((overiva_k<M, K>), dim3((unsigned)B), dim3(OverivaGeom<M, K>::THREADS), 0, s, a);
}

hipError_t launch_overiva(const void* mix, int B, int M, int K, int T, int F, int model, int ref_ch, double alpha, double floor,
                          void* est, void* images, void* state, hipStream_t s) {
  if (M < 2 || M > 8 || K < 1 || K >= M || F < 1 || F > OVERIVA_FMAX) return hipErrorInvalidValue;
  OverivaArgs a;
  a.mix = reinterpret_cast<const float2*>(mix);
  a.est = reinterpret_cast<float2*>(est);
  a.img = reinterpret_cast<float2*>(images);
  a.state = reinterpret_cast<char*>(state);
  a.w = overiva_ws((long long)B * F, M, K);
  a.T = T; a.F = F; a.model = model; a.ref = ref_ch;
  a.alpha = alpha; a.oma = 1.0 - alpha; a.floor = floor;
  with_mk(M, K, [&](auto m, auto k) { overiva_go<decltype(m)::value, decltype(k)::value>(a, B, s); });
  return hipGetLastError();
}

hipError_t launch_overiva_debug(const void* state, int B, int M, int K, int F, void* ws, void* jm, void* v, void* c, int* fail,
                                int* n, hipStream_t s) {
  const long long bins = (long long)B * F;
  const OverivaWs w = overiva_ws(bins, M, K);
  return copy_parts(state, {{ws, w.W, bins * K * M * 16}, {jm, w.J, bins * (M - K) * K * 16}, {v, w.V, bins * K * M * M * 16},
                            {c, w.C, bins * M * M * 16}, {fail, w.fail, bins * 4}, {n, w.n, bins * 4}}, s);
}

}  // namespace mn
