// What the two online AuxIVA kernel files share (oiva.hip, overiva.hip): the load of a frame's samples of one bin and the
// elimination over the rows held by the lanes of a group.  Kernel files only; one definition of each.  The text is what oiva.hip
// held: its kernels compile to the instructions they compiled to before the move (the device assembly of the file, compared).
#pragma once
#include "cplx.hpp"

namespace mn {

// the frame's M samples of one bin (widened where they are used); true when one of them is not finite (they then count as 0)
template <int M> __device__ __forceinline__ bool oiva_load(const float2* p, long long stride, float2 (&x)[M]) {
  bool bad = false;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float2 v = p[m * stride];
    bad |= !(finite(v.x) && finite(v.y));
    x[m] = v;
  }
  if (bad) {
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = make_float2(0.f, 0.f);
  }
  return bad;
}

// Gaussian elimination with partial pivoting over the rows held by the lanes of a group, then back substitution.  Lane j < M
// holds row j of the matrix (A) and of the R right-hand sides (rhs); both are destroyed.  take(c, r, v) is called for c = M - 1
// .. 0 and r = 0 .. R - 1 with entry (c, r) of the solution, the same on every lane.  Returns true when a pivot was 0 or not finite.
template <int M, int G, int R, class Take>
__device__ __forceinline__ bool oiva_solve(double2 (&A)[M], double2 (&rhs)[R], int j, Take&& take) {
  int pos = j;                                                         // the position of this lane's row; lanes >= M never move
  int pl[M];                                                           // the lane that holds the row at position c
  bool bad = false;
#pragma unroll
  for (int c = 0; c < M; ++c) {
    double bm = fabs(A[c].x) + fabs(A[c].y);
    if (!(bm <= F64_MAX)) bm = __builtin_inf();                        // a non-finite one counts as the largest: it is flagged
    if (j >= M || pos < c) bm = -1.0;
    int bp = pos, bl = j;
#pragma unroll
    for (int s = 1; s < G; s <<= 1) {                                  // the largest; of equal ones the lower position
      const double om = __shfl_xor(bm, s, G);
      const int op = __shfl_xor(bp, s, G), ol = __shfl_xor(bl, s, G);
      if (om > bm || (om == bm && op < bp)) { bm = om; bp = op; bl = ol; }
    }
    bad |= !(bm > 0.0 && bm <= F64_MAX);
    if (j == bl) pos = c;                                              // the rows at c and at bp change places
    else if (pos == c) pos = bp;
    pl[c] = bl;
    const double2 ip = c_inv(c_from<G>(A[c], bl));
    const bool below = j < M && pos > c;
    const double2 l = c_mul(A[c], ip);
#pragma unroll
    for (int cc = c + 1; cc < M; ++cc) {
      const double2 pr = c_from<G>(A[cc], bl);
      if (below) A[cc] = c_fms(A[cc], l, pr);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double2 pr = c_from<G>(rhs[r], bl);
      if (below) rhs[r] = c_fms(rhs[r], l, pr);
    }
    __builtin_amdgcn_sched_barrier(0);                                 // one column at a time, for the registers' sake
  }
#pragma unroll
  for (int c = M - 1; c >= 0; --c) {
    double2 xc[R];
    const bool above = j < M && pos < c;
    const double2 ip = c_inv(A[c]);                                 // the pivot on the lane that holds row c; unused elsewhere
#pragma unroll
    for (int r = 0; r < R; ++r) {
      xc[r] = c_from<G>(c_mul(rhs[r], ip), pl[c]);
      if (above) rhs[r] = c_fms(rhs[r], A[c], xc[r]);
      take(c, r, xc[r]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return bad;
}

}  // namespace mn
