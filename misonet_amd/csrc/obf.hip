// Online beamformer (recursive Souden MVDR / rank-1 SDW-MWF; Souden, Benesty & Affes 2010 for the filter, Higuchi et al. 2017 and
// Boeddeker et al. 2018 for the recursive use) on the device: C ABI misonet_obf* in api_array.hip; the definition is
// INTEGRATION.md 4t and is restated in NumPy in tests/obf_ref.py.
//
// Every cell (item b, source s, bin f) runs on its own.  Its state is Phi_s and Phi_n [M][M] complex128 (Hermitian), the filter w
// [M] of the last frame (stored, never read by the recursion), the frame count n and the fail word.  Per new frame, y the M
// samples of mix and x those of images[b, s], float64 after the loads:
//
//   0. a non-finite sample in y or x: fail |= 1, Phi_s, Phi_n and w stay, out = 0
//   1. v = y - x (noise 0 "residual") or v = y (noise 1 "mix")
//   2. Phi_s <- alpha Phi_s + (1 - alpha) x x^H, Phi_n <- alpha Phi_n + (1 - alpha) v v^H: the lower triangle, mirrored, diagonal real
//   3. R = Phi_n + (diag_load tr(Phi_n) / M + epsi) I
//   4. R = L L^H column by column; a pivot not finite or not > 0: fail |= 2, w = 0, out = 0 (the Phi of step 2 stay)
//   5. G = R^-1 Phi_s by the two triangular solves, den = mu + sum_m G[m][m]; den not finite: fail |= 4, w = 0, out = 0; den == 0:
//      w = 0, out = 0, no flag; otherwise w = G[:, ref] (1 / den), the reciprocal in Smith's form
//   6. out = sum_m conj(w_m) y_m, rounded once to complex64
//   7. n <- n + 1 (it stops at 2^31 - 1)
//
//   obf_reset_k  every 16 bytes of the state: Phi_n = init I, the rest 0
//   obf_k<M>     the cells (b, s, f) are flattened over the grid; a group of G = 2, 4 or 8 lanes (the power of two that holds M)
//                owns a cell, one wave (ObfGeom<M>::CELLS = 64 / G cells) is a workgroup and walks the T frames of its cells in
//                order.  Nothing couples the cells: no barrier, no LDS.  Lane j holds row j of Phi_s, Phi_n, L and of the
//                right-hand sides in registers for the whole call: the state is loaded once and written back once.  The samples
//                of frame t + 1 are loaded before frame t is solved.  M is a template parameter: every matrix index is a constant.
//                  - step 2: entry (j, c) is formed as entry (max, min) of the lower triangle -- on lane j and on lane c from the
//                    same operands (the stored matrix being Hermitian to the bit), without fused multiply-adds -- and conjugated
//                    where c > j: the matrices stay exactly Hermitian.
//                  - step 4: left-looking; for column c the first c entries of row c come from lane c by __shfl, lane j keeps
//                    L[c][j] (column j of L, for the second solve) as they pass; the pivot comes from lane c; 1 / L[c][c] is kept
//                    and multiplies where the definition divides by L[c][c].
//                  - step 5: L Z = Phi_s for all M columns, row c finished on lane c and broadcast, rows below updated (for row j
//                    the terms are subtracted with k ascending); L^H G = Z from the last row up (k descending), for the columns
//                    r <= c that the trace still needs and for column ref.  G[c][c] and G[c][ref] are read off the broadcast.
//
// Every sum has one fixed order that depends on M only; no atomics, no scratch: the result is bit-reproducible, does not depend
// on the batch or the position in it, and -- the state being all that passes from one frame to the next, as exact float64 --
// does not depend on how the stream is cut into calls.  One launch, no host synchronisation, no allocation; nothing in the
// launch or the state depends on T.
#include "kernels.hpp"
#include "cplx.hpp"

namespace mn {

template <int M> struct ObfGeom {
  static constexpr int G = lanes_for(M);                               // lanes per cell
  static constexpr int THREADS = 64;                                   // one wave: the cells spread over as many CUs as there are
  static constexpr int CELLS = THREADS / G;                            // cells per workgroup: 32, 16, 16, 8, 8, 8, 8
};

int obf_cells_per_block(int M) {
  int cells = -1;
  if (M >= 2 && M <= 8) with_m(M, [&](auto m) { cells = ObfGeom<decltype(m)::value>::CELLS; });
  return cells;
}

// state: fail int [cells] | n int [cells] | Phi_s c128 [cells][M][M] | Phi_n c128 [cells][M][M] | w c128 [cells][M]
struct ObfWs { long long fail, n, ps, pn, w, total; };
__host__ __device__ inline ObfWs obf_ws(long long cells, int M) {
  ObfWs w;
  w.fail = 0;
  w.n = align16(cells * 4);
  w.ps = align16(w.n + cells * 4);
  w.pn = w.ps + cells * M * M * 16;
  w.w = w.pn + cells * M * M * 16;
  w.total = w.w + cells * M * 16;
  return w;
}
long long obf_state_bytes(long long cells, int M) { return obf_ws(cells, M).total; }

struct ObfArgs {
  const float2 *mix, *img;
  float2* out;
  char* state;
  ObfWs w;
  long long cells;
  int S, T, F, noise, ref;
  double alpha, oma, mu, diag_load, epsi;                              // oma = 1 - alpha
};

// frame t of a cell: the M samples of the source image and of the mixture, as they lie (strided in m, contiguous in f)
template <int M>
__device__ __forceinline__ void obf_load(const float2* xp, const float2* yp, long long stride, long long at, float2 (&x)[M],
                                         float2 (&y)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    x[m] = xp[m * stride + at];
    y[m] = yp[m * stride + at];
  }
}

// row jr of P <- alpha P + oma u u^H, formed as the lower-triangle entry (max(jr, c), min(jr, c)) and conjugated where c > jr; uj = u[jr]
template <int M>
__device__ __forceinline__ void obf_update(double2 (&P)[M], const double2 (&u)[M], double2 uj, int jr, double alpha, double oma,
                                           bool keep) {
  // No fused multiply-add in here.  Entry (j, c) on lane j and entry (c, j) on lane c come from different unrolled rounds, and
  // the compiler sees through the selects below; with every product rounded on its own the two agree to the bit however it
  // orders them (rounding is symmetric in the sign, products commute) -- a fused a b - c d is not the negative of c d - a b.
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < M; ++c) {
    const bool lower = jr >= c;
    const double2 a = c_sel(lower, uj, u[c]), b = c_sel(lower, u[c], uj), o = P[c];
    const double oy = lower ? o.y : -o.y;
    const double re = alpha * o.x + oma * (a.x * b.x + a.y * b.y);
    double im = alpha * oy + oma * (a.y * b.x - a.x * b.y);
    im = jr == c ? 0.0 : lower ? im : -im;
    P[c] = c_sel(keep, o, make_double2(re, im));
  }
}

// grid (ceil(total / 16 / 256)), 256 threads: every 16 bytes of the state
__global__ __launch_bounds__(256) void obf_reset_k(char* state, long long cells, int M, double init) {
  const ObfWs w = obf_ws(cells, M);
  const long long units = w.total / 16, nm = cells * M * M;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
    const long long off = u * 16;
    double2 v = make_double2(0.0, 0.0);
    if (off >= w.pn && off < w.w) {
      const long long e = (off - w.pn) / 16;
      if (e < nm && (e / M) % M == e % M) v.x = init;
    }
    *reinterpret_cast<double2*>(state + off) = v;
  }
}

// grid (ceil(cells / ObfGeom<M>::CELLS)), ObfGeom<M>::THREADS threads
template <int M>
__global__ __launch_bounds__(ObfGeom<M>::THREADS) void obf_k(const ObfArgs a) {
  constexpr int G = ObfGeom<M>::G, CELLS = ObfGeom<M>::CELLS;
  const int tid = threadIdx.x, j = tid & (G - 1), slot = tid / G;
  const long long cell = (long long)blockIdx.x * CELLS + slot;
  const bool act = cell < a.cells, row = j < M;
  const long long cc = act ? cell : a.cells - 1;                       // an idle group repeats the last cell and stores nothing
  const int jr = row ? j : M - 1;                                      // an idle lane of a group repeats row M - 1 and stores nothing
  const unsigned jbit = 1u << jr;                                      // an entry that jr names is picked by a chain of selects
  const int T = a.T, F = a.F, ref = a.ref;
  const long long TF = (long long)T * F, bs = cc / F, f = cc - bs * F, b = bs / a.S;
  const float2* yp = a.mix + b * M * TF + f;                           // frame t of microphone m: yp[m TF + t F]
  const float2* xp = a.img + bs * M * TF + f;
  float2* op = a.out + bs * TF + f;
  int* failp = reinterpret_cast<int*>(a.state + a.w.fail) + cc;
  int* np = reinterpret_cast<int*>(a.state + a.w.n) + cc;
  double2* psg = reinterpret_cast<double2*>(a.state + a.w.ps) + (cc * M + jr) * M;
  double2* png = reinterpret_cast<double2*>(a.state + a.w.pn) + (cc * M + jr) * M;
  double2* wg = reinterpret_cast<double2*>(a.state + a.w.w) + cc * M;
  const double alpha = a.alpha, oma = a.oma;
  const bool residual = a.noise == 0;

  double2 Ps[M], Pn[M], W[M];
#pragma unroll
  for (int c = 0; c < M; ++c) { Ps[c] = psg[c]; Pn[c] = png[c]; W[c] = wg[c]; }
  int flags = 0;
  float2 xn[M], yn[M];
  obf_load<M>(xp, yp, TF, 0, xn, yn);

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    // the lane's row number, opaque and made anew in every frame and before every step: the masks of its comparisons would
    // otherwise be kept in SGPRs across the whole frame loop, and spill
    int jk = jr;
    asm volatile("" : "+v"(jk));
    unsigned kbit = 1u << jk;
    float2 x[M], y[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { x[m] = xn[m]; y[m] = yn[m]; }
    obf_load<M>(xp, yp, TF, (long long)(t + 1 < T ? t + 1 : t) * F, xn, yn);   // the next frame, while this one is solved

    // ---- 0, 1. the frame's vectors; a bad frame runs on as zeros and changes nothing
    bool bad = false;
#pragma unroll
    for (int m = 0; m < M; ++m) bad |= !(finite(x[m].x) && finite(x[m].y) && finite(y[m].x) && finite(y[m].y));
    double2 xd[M], yd[M], vd[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double2 zero = make_double2(0.0, 0.0);
      xd[m] = c_sel(bad, zero, c_wide(x[m]));
      yd[m] = c_sel(bad, zero, c_wide(y[m]));
      vd[m] = c_sel(residual, make_double2(yd[m].x - xd[m].x, yd[m].y - xd[m].y), yd[m]);
    }
    double2 xj = xd[0], vj = vd[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
      const bool mine = kbit >> m & 1u;
      xj = c_sel(mine, xd[m], xj);
      vj = c_sel(mine, vd[m], vj);
    }

    // ---- 2. the covariances
    obf_update<M>(Ps, xd, xj, jk, alpha, oma, bad);
    obf_update<M>(Pn, vd, vj, jk, alpha, oma, bad);

    // ---- 3. R = Phi_n + load I: row jk
    double dn = Pn[0].x;
#pragma unroll
    for (int m = 1; m < M; ++m)
      if (kbit >> m & 1u) dn = Pn[m].x;
    double tr = __shfl(dn, 0, G);
#pragma unroll
    for (int m = 1; m < M; ++m) tr += __shfl(dn, m, G);
    const double load = a.diag_load * tr / (double)M + a.epsi;

    asm volatile("" : "+v"(jk));
    kbit = 1u << jk;
    // ---- 4. R = L L^H, left-looking: Lr row jk of L (below the diagonal), Lc[c] = L[c][jk], invd[c] = 1 / L[c][c]
    double2 Lr[M], Lc[M];
    double invd[M];
    bool pbad = false;
#pragma unroll
    for (int c = 0; c < M; ++c) Lc[c] = make_double2(0.0, 0.0);
#pragma unroll
    for (int c = 0; c < M; ++c) {
      double2 s = Pn[c];
      if (jk == c) s.x += load;
#pragma unroll
      for (int k = 0; k < c; ++k) {
        const double2 bc = c_from<G>(Lr[k], c);                      // L[c][k]
        s = c_fmsc(s, Lr[k], bc);
        Lc[c] = c_sel(kbit >> k & 1u, bc, Lc[c]);
      }
      const double p = __shfl(s.x, c, G);
      pbad |= !(p > 0.0 && p <= F64_MAX);
      const double inv = 1.0 / sqrt(p);
      invd[c] = inv;
      Lr[c] = make_double2(s.x * inv, s.y * inv);
    }

    asm volatile("" : "+v"(jk));
    kbit = 1u << jk;
    // ---- 5. L Z = Phi_s: row c is finished on lane c and goes to all
    double2 rhs[M];
#pragma unroll
    for (int r = 0; r < M; ++r) rhs[r] = Ps[r];
#pragma unroll
    for (int c = 0; c < M; ++c) {
#pragma unroll
      for (int r = 0; r < M; ++r) {
        const double2 zb = c_from<G>(make_double2(rhs[r].x * invd[c], rhs[r].y * invd[c]), c);
        const double2 below = c_fms(rhs[r], Lr[c], zb);
        rhs[r] = c_sel(jk > c, below, c_sel(jk == c, zb, rhs[r]));
      }
    }
    asm volatile("" : "+v"(jk));
    kbit = 1u << jk;
    // L^H G = Z from the last row up: the columns r <= c (for the trace) and column ref
    double2 zr = rhs[0];
#pragma unroll
    for (int r = 1; r < M; ++r)
      zr = c_sel(ref == r, rhs[r], zr);
    double2 gd[M], gref[M];
#pragma unroll
    for (int c = M - 1; c >= 0; --c) {
      const bool above = jk < c;
      const double2 lc = make_double2(Lc[c].x, -Lc[c].y);              // conj(L[c][jk])
#pragma unroll
      for (int r = 0; r <= c; ++r) {
        const double2 gb = c_from<G>(make_double2(rhs[r].x * invd[c], rhs[r].y * invd[c]), c);
        if (r == c) gd[c] = gb;
        const double2 up = c_fms(rhs[r], lc, gb);
        rhs[r] = c_sel(above, up, rhs[r]);
      }
      const double2 gb = c_from<G>(make_double2(zr.x * invd[c], zr.y * invd[c]), c);
      gref[c] = gb;
      const double2 up = c_fms(zr, lc, gb);
      zr = c_sel(above, up, zr);
    }
    double2 acc = gd[0];
#pragma unroll
    for (int m = 1; m < M; ++m) acc = make_double2(acc.x + gd[m].x, acc.y + gd[m].y);
    const double2 den = make_double2(a.mu + acc.x, acc.y);
    const bool fin = finite(den.x) && finite(den.y);
    const bool zero = den.x == 0.0 && den.y == 0.0;
    const double2 iden = c_inv(den);
    const bool ok = !bad && !pbad && fin && !zero;
    if (bad) flags |= 1;
    else if (pbad) flags |= 2;
    else if (!fin) flags |= 4;

    // ---- 6. the filter and the output
    double2 o = make_double2(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double2 wn = c_mul(gref[m], iden);
      W[m] = c_sel(bad, W[m], c_sel(ok, wn, make_double2(0.0, 0.0)));
      o.x += W[m].x * yd[m].x + W[m].y * yd[m].y;                      // conj(w) y
      o.y += W[m].x * yd[m].y - W[m].y * yd[m].x;
    }
    if (act && j == 0) op[(long long)t * F] = ok ? make_float2((float)o.x, (float)o.y) : make_float2(0.f, 0.f);
  }

  // ---- the state goes back once; 7. the frames seen
  if (act && row) {
#pragma unroll
    for (int c = 0; c < M; ++c) { psg[c] = Ps[c]; png[c] = Pn[c]; }
    double2 wj = W[0];
#pragma unroll
    for (int m = 1; m < M; ++m)
      wj = c_sel(jbit >> m & 1u, W[m], wj);
    wg[j] = wj;
  }
  if (act && j == 0) {
    if (flags) *failp |= flags;
    const long long n = (long long)*np + T;
    *np = n < 0x7fffffffLL ? (int)n : 0x7fffffff;
  }
}

hipError_t launch_obf_reset(void* state, int B, int S, int M, int F, double init, hipStream_t s) {
  const long long cells = (long long)B * S * F, units = obf_state_bytes(cells, M) / 16;
  const long long blocks = (units + 255) / 256;
  hipLaunchKernelGGL(obf_reset_k, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, reinterpret_cast<char*>(state),
                     cells, M, init);
  return hipGetLastError();
}

template <int M> static void obf_go(const ObfArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(obf_k<M>, dim3((unsigned)((a.cells + ObfGeom<M>::CELLS - 1) / ObfGeom<M>::CELLS)), dim3(ObfGeom<M>::THREADS), 0, s, a);
}

hipError_t launch_obf(const void* mix, const void* images, int B, int S, int M, int T, int F, int noise, int ref_ch, double alpha,
                      double mu, double diag_load, double epsi, void* out, void* state, hipStream_t s) {
  if (M < 2 || M > 8 || S < 1 || B < 1 || F < 1 || T < 1 || ref_ch < 0 || ref_ch >= M) return hipErrorInvalidValue;
  ObfArgs a;
  a.mix = reinterpret_cast<const float2*>(mix);
  a.img = reinterpret_cast<const float2*>(images);
  a.out = reinterpret_cast<float2*>(out);
  a.state = reinterpret_cast<char*>(state);
  a.cells = (long long)B * S * F;
  a.w = obf_ws(a.cells, M);
  a.S = S; a.T = T; a.F = F; a.noise = noise; a.ref = ref_ch;
  a.alpha = alpha; a.oma = 1.0 - alpha; a.mu = mu; a.diag_load = diag_load; a.epsi = epsi;
  with_m(M, [&](auto m) { obf_go<decltype(m)::value>(a, s); });
  return hipGetLastError();
}

hipError_t launch_obf_debug(const void* state, int B, int S, int M, int F, void* phi_s, void* phi_n, void* w, int* fail, int* n,
                            hipStream_t s) {
  const long long cells = (long long)B * S * F;
  const ObfWs ws = obf_ws(cells, M);
  return copy_parts(state, {{phi_s, ws.ps, cells * M * M * 16}, {phi_n, ws.pn, cells * M * M * 16}, {w, ws.w, cells * M * 16},
                            {fail, ws.fail, cells * 4}, {n, ws.n, cells * 4}}, s);
}

}  // namespace mn
