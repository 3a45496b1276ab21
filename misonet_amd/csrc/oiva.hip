// Online AuxIVA (Taniguchi, Ono, Kawamura & Sagayama 2014) on the device: C ABI misonet_oiva* in api_array.hip; the definition
// is INTEGRATION.md 4s and is restated in NumPy in tests/oiva_ref.py.
//
// The determined case, K = M.  The state of (item b, bin f) is W [M][M] (row k = w_k^H, y = W x) and V [M][M][M] complex128 (one
// Hermitian matrix per source), the frame count n and the fail word.  Per new frame, float64 after the load:
//
//   0. a bin whose frame holds a non-finite sample: fail |= 1, x = 0 below, step 3 skipped, its outputs 0
//   1. yt_k[f] = sum_m W_f[k][m] x_f[m]                      W as it stood before the frame
//   2. r_k = sum_f |yt_k[f]|^2,  phi_k = 1 / max(r_k / F, floor) (gauss) or 1 / max(2 sqrt(r_k), floor) (laplace)
//   3. per bin, k = 0 .. M - 1:  V_k <- alpha V_k + (1 - alpha) phi_k x x^H,  (W V_k) u = e_k,  d = Re(u^H V_k u),
//      row k of W <- conj(u) / sqrt(d); a pivot 0 or non-finite, d not finite or not > 0: the row stays, fail |= 2
//   4. y = W x, A = W^-1, est[k] = A[ref][k] y_k, images[k][m] = A[m][k] y_k; W singular: fail |= 4, outputs 0
//   5. n <- n + 1 (it stops at 2^31 - 1)
//
//   oiva_reset_k  every 16 bytes of the state: W = I, V_k = init I, the rest 0
//   oiva_k<M>     one workgroup per item walks the T frames of the call in order, because step 2 couples all bins of an item
//                 once per frame: two barriers per frame, one behind |yt|^2 and one behind phi; no workgroup ever waits for
//                 another.  A group of G = 2, 4 or 8 lanes (the power of two that holds M) owns a bin, lane j row j of W, of
//                 W V_k and of V_k; a workgroup covers OivaGeom<M>::BINS bins at once and walks ceil(F / BINS) passes.  The state
//                 does not fit the LDS (M = 6, F = 129: 0.6 MB), so it is read from and written back to global memory in every
//                 frame -- it stays in L2; the LDS holds only |yt|^2 [M][F] and phi.  M is a template parameter: every matrix
//                 index is a constant and the kernel uses no scratch.  The workgroup is as large as the registers of the rows
//                 allow (OivaGeom): 1024 threads at M = 2, 768 at 3, 512 at 4 and 5, 256 from 6 on (one wave per SIMD, with
//                 AGPRs behind the VGPRs).
//                   - V_k: every lane of the group forms the whole updated matrix from the stored lower triangle (the same
//                     instructions on the same operands: the same bits on every lane), the upper triangle is its conjugate and
//                     the diagonal's imaginary part is set to 0, so the stored V_k is exactly Hermitian; lane j keeps row j.
//                   - the elimination: partial pivoting by a butterfly over the group on (|re| + |im|, row position), the pivot
//                     row broadcast with __shfl, rows exchanged by exchanging their positions; back substitution column by
//                     column, each solved entry broadcast from the lane that holds its row.
//                   - step 2: wave k adds |yt_k[f]|^2 over f = lane, lane + 64, ... and then over the 64 lanes by a butterfly:
//                     one order, fixed by F alone.
//
// Every sum has one fixed order that depends on M and F only and nothing is accumulated with atomics: the result is
// bit-reproducible, does not depend on the batch or the position in it, and -- the state being all that passes from one frame to
// the next -- does not depend on how the stream is cut into calls.  One launch, no host synchronisation, no allocation; nothing
// in the launch or the state depends on T.
#include "kernels.hpp"
#include "cplx.hpp"
#include "oiva_solve.hpp"

namespace mn {

constexpr int OIVA_FMAX = 1025;

template <int M> struct OivaGeom {
  static constexpr int G = lanes_for(M);                               // lanes per bin
  // 4, 3, 2 or 1 waves per SIMD: 128, 168, 256 or 512 registers each, what the rows of W, W V_k, V_k and u of that M take
  static constexpr int THREADS = M <= 2 ? 1024 : M <= 3 ? 768 : M <= 5 ? 512 : 256;
  static constexpr int BINS = THREADS / G;                             // bins per pass: 512, 192, 128, 64, 32, 32, 32
};

int oiva_bins_per_pass(int M) {
  int bins = -1;
  if (M >= 2 && M <= 8) with_m(M, [&](auto m) { bins = OivaGeom<decltype(m)::value>::BINS; });
  return bins;
}

// state: fail int [bins] | n int [bins] | W c128 [bins][M][M] | V c128 [bins][M][M][M]
struct OivaWs { long long fail, n, W, V, total; };
__host__ __device__ inline OivaWs oiva_ws(long long bins, int M) {
  OivaWs w;
  w.fail = 0;
  w.n = align16(bins * 4);
  w.W = align16(w.n + bins * 4);
  w.V = w.W + bins * M * M * 16;
  w.total = w.V + bins * M * M * M * 16;
  return w;
}
long long oiva_state_bytes(long long bins, int M) { return oiva_ws(bins, M).total; }

struct OivaArgs {
  const float2* mix;
  float2 *est, *img;
  char* state;
  OivaWs w;
  int T, F, model, ref;
  double alpha, oma, floor;                                            // oma = 1 - alpha
};

// grid (ceil(total / 16 / 256)), 256 threads: every 16 bytes of the state
__global__ __launch_bounds__(256) void oiva_reset_k(char* state, long long bins, int M, double init) {
  const OivaWs w = oiva_ws(bins, M);
  const long long units = w.total / 16, nw = bins * M * M, nv = nw * M;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
    const long long off = u * 16;
    double2 v = make_double2(0.0, 0.0);
    if (off >= w.V) {
      const long long e = (off - w.V) / 16;
      if (e < nv && (e / M) % M == e % M) v.x = init;
    } else if (off >= w.W) {
      const long long e = (off - w.W) / 16;
      if (e < nw && (e / M) % M == e % M) v.x = 1.0;
    }
    *reinterpret_cast<double2*>(state + off) = v;
  }
}

// grid (B), OivaGeom<M>::THREADS threads
template <int M>
__global__ __launch_bounds__(OivaGeom<M>::THREADS) void oiva_k(const OivaArgs a) {
  constexpr int G = OivaGeom<M>::G, THREADS = OivaGeom<M>::THREADS, BINS = OivaGeom<M>::BINS;
  __shared__ double part[M * OIVA_FMAX];                               // |yt_k[f]|^2 at [k][f]
  __shared__ double phil[8];

  const int T = a.T, F = a.F;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = tid & (G - 1), slot = tid / G;
  const bool row = j < M;
  // An entry of a register array that a run-time index names (the lane's own column, ref_ch) is picked by a chain of tests on one
  // opaque bit each: a chain of comparisons with the index becomes an indexed load, and the array scratch
  unsigned rbit = 1u << a.ref;
  asm volatile("" : "+s"(rbit));
  const int jr = row ? j : M - 1;                                      // the row an idle lane of the group reads (and never writes)
  const long long bin0 = (long long)b * F, TF = (long long)T * F;
  int* failp = reinterpret_cast<int*>(a.state + a.w.fail) + bin0;
  int* np = reinterpret_cast<int*>(a.state + a.w.n) + bin0;
  double2* Wg = reinterpret_cast<double2*>(a.state + a.w.W) + bin0 * M * M;
  double2* Vg = reinterpret_cast<double2*>(a.state + a.w.V) + bin0 * M * M * M;
  const float2* xb = a.mix + (long long)b * M * TF;                    // frame t of microphone m: xb[(m T + t) F + f]
  float2* eb = a.est + (long long)b * M * TF;
  float2* ib = a.img ? a.img + (long long)b * M * M * TF : nullptr;
  const double alpha = a.alpha, oma = a.oma;

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    // ---- 1. |yt|^2 of every bin with W as it stands
#pragma unroll 1
    for (int f0 = 0; f0 < F; f0 += BINS) {
      const int f = f0 + slot;
      const bool act = f < F;
      const int fc = act ? f : F - 1;
      float2 x[M];
      oiva_load<M>(xb + (long long)t * F + fc, TF, x);
      const double2* wr = Wg + ((long long)fc * M + jr) * M;
      double2 y = make_double2(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) y = c_fma(y, wr[m], c_wide(x[m]));
      if (act && row) part[j * OIVA_FMAX + f] = y.x * y.x + y.y * y.y;
    }
    __syncthreads();

    // ---- 2. r_k over the bins in one fixed order, phi_k
    for (int k = wave; k < M; k += THREADS / 64) {
      double s = 0.0;
      for (int f = lane; f < F; f += 64) s += part[k * OIVA_FMAX + f];
#pragma unroll
      for (int q = 32; q >= 1; q >>= 1) s += __shfl_xor(s, q, 64);
      if (lane == 0) phil[k] = 1.0 / fmax(a.model == 0 ? s / (double)F : 2.0 * sqrt(s), a.floor);
    }
    __syncthreads();

    // ---- 3 - 5. per bin: the covariances, the rows of W, the outputs
#pragma unroll 1
    for (int f0 = 0; f0 < F; f0 += BINS) {
      const int f = f0 + slot;
      const bool act = f < F;
      const int fc = act ? f : F - 1;
      float2 x[M];
      double2 Wr[M];
      const bool bad = oiva_load<M>(xb + (long long)t * F + fc, TF, x);
      double2* wr = Wg + ((long long)fc * M + jr) * M;
#pragma unroll
      for (int m = 0; m < M; ++m) Wr[m] = wr[m];
      const bool upd = act && !bad;
      int flags = bad ? 1 : 0;

#pragma unroll 1
      for (int k = 0; k < M; ++k) {
        // the lane's row number, opaque and made anew in every round: the masks of its comparisons would otherwise be kept in
        // SGPRs across the whole frame loop, and spill
        int jk = j;
        asm volatile("" : "+v"(jk));
        const unsigned jbit = 1u << jk;
        const double g = oma * phil[k];
        double2* vk = Vg + ((long long)fc * M + k) * M * M;
        double2 Tr[M], Vr[M];                                          // row j of W V_k and of V_k
#pragma unroll
        for (int c = 0; c < M; ++c) { Tr[c] = make_double2(0.0, 0.0); Vr[c] = Tr[c]; }
#pragma unroll
        for (int m = 0; m < M; ++m) {
#pragma unroll
          for (int c = 0; c <= m; ++c) {                               // the lower triangle; the upper is its conjugate
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
          __builtin_amdgcn_sched_barrier(0);                           // one row at a time: the loads of all rows at once spill
        }
        if (upd && row) {
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
        for (int s = 1; s < G; s <<= 1) d += __shfl_xor(d, s, G);      // the same bits on every lane of the group
        const bool ok = !sbad && d > 0.0 && d <= F64_MAX;
        if (!ok && !bad) flags |= 2;
        if (ok && jk == k) {
          const double inv = 1.0 / sqrt(d);
#pragma unroll
          for (int c = 0; c < M; ++c) Wr[c] = make_double2(u[c].x * inv, -u[c].y * inv);
        }
      }
      if (upd && row) {
#pragma unroll
        for (int c = 0; c < M; ++c) wr[c] = Wr[c];
      }

      // ---- 4. y = W x, A = W^-1: lane k takes column k of A as the rows of the solution come by
      double2 y = make_double2(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) y = c_fma(y, Wr[m], c_wide(x[m]));
      double2 eye[M], acol[M];
      int ja = j;
      asm volatile("" : "+v"(ja));
      const unsigned jbit = 1u << ja;
#pragma unroll
      for (int c = 0; c < M; ++c) eye[c] = make_double2(c == ja ? 1.0 : 0.0, 0.0);
      const bool abad = oiva_solve<M, G, M>(Wr, eye, ja, [&](int c, int r, double2 v) __attribute__((always_inline)) {
        if (r == 0 || (jbit >> r & 1u)) acol[c] = v;
      });
      if (abad && !bad) flags |= 4;
      const bool zero = bad || abad;
      if (act && row) {
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
      if (act && j == 0) {
        if (flags) failp[f] |= flags;
        const int n = np[f];
        if (n < 0x7fffffff) np[f] = n + 1;
      }
    }
  }
}

hipError_t launch_oiva_reset(void* state, int B, int M, int F, double init, hipStream_t s) {
  const long long bins = (long long)B * F, units = oiva_state_bytes(bins, M) / 16;
  const long long blocks = (units + 255) / 256;
  hipLaunchKernelGGL(oiva_reset_k, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, reinterpret_cast<char*>(state),
                     bins, M, init);
  return hipGetLastError();
}

template <int M> static void oiva_go(const OivaArgs& a, int B, hipStream_t s) {
  hipLaunchKernelGGL(oiva_k<M>, dim3((unsigned)B), dim3(OivaGeom<M>::THREADS), 0, s, a);
}

hipError_t launch_oiva(const void* mix, int B, int M, int T, int F, int model, int ref_ch, double alpha, double floor, void* est,
                       void* images, void* state, hipStream_t s) {
  if (M < 2 || M > 8 || F < 1 || F > OIVA_FMAX) return hipErrorInvalidValue;
  OivaArgs a;
  a.mix = reinterpret_cast<const float2*>(mix);
  a.est = reinterpret_cast<float2*>(est);
  a.img = reinterpret_cast<float2*>(images);
  a.state = reinterpret_cast<char*>(state);
  a.w = oiva_ws((long long)B * F, M);
  a.T = T; a.F = F; a.model = model; a.ref = ref_ch;
  a.alpha = alpha; a.oma = 1.0 - alpha; a.floor = floor;
  with_m(M, [&](auto m) { oiva_go<decltype(m)::value>(a, B, s); });
  return hipGetLastError();
}

hipError_t launch_oiva_debug(const void* state, int B, int M, int F, void* w, void* v, int* fail, int* n, hipStream_t s) {
  const long long bins = (long long)B * F;
  const OivaWs ws = oiva_ws(bins, M);
  return copy_parts(state, {{w, ws.W, bins * M * M * 16}, {v, ws.V, bins * M * M * M * 16}, {fail, ws.fail, bins * 4},
                            {n, ws.n, bins * 4}}, s);
}

}  // namespace mn
