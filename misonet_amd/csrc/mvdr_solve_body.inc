// The body of mvdr_solve<M> and of mvdr_solve_ext<M> (mvdr.hip includes it into both).  In scope: M, EXT, B, S, F, epsi, ws
// and, where EXT, cond, tn, ban.
  extern __shared__ double s_d[];     // [F][M][2]
  const int b = blockIdx.x, spk = blockIdx.y;
  const int tid = threadIdx.x;
  const long long base = (long long)(b * S + spk) * F;
  const double* d0 = ws + ws_steer0(B, S, F, M) + base * (M * 2);
  for (int i = tid; i < F * M * 2; i += blockDim.x) s_d[i] = d0[i];
  __syncthreads();
  // sequential-in-f phase correction (tester.py:1161-1167): bin f is rotated by the phase of <d[f], d_corrected[f-1]>.
  // The dependence from bin to bin is kept exactly; inside a bin lane m < M owns microphone m (the M products and the M
  // rotations run on M lanes, the sum over m is a butterfly over 8 lanes with zeros in the unused ones).
  if (tid < 8) {
    const int m = tid;
    const bool live = m < M;
    cd prv = live ? cd{s_d[m * 2], s_d[m * 2 + 1]} : cd{0.0, 0.0};
    for (int f = 1; f < F; ++f) {
      const cd cur = live ? cd{s_d[(f * M + m) * 2], s_d[(f * M + m) * 2 + 1]} : cd{0.0, 0.0};
      cd z = cmulc(cur, prv);
#pragma unroll
      for (int w = 4; w >= 1; w >>= 1) {
        z.re += __shfl_xor(z.re, w, 8);
        z.im += __shfl_xor(z.im, w, 8);
      }
      const double az = sqrt(cabs2(z));
      cd rot = {1.0, 0.0};                                // exp(-j angle(z)); angle(0) = 0
      if (az > 0.0) rot = {z.re / az, -z.im / az};
      prv = cmul(cur, rot);
      if (live) {
        s_d[(f * M + m) * 2] = prv.re;
        s_d[(f * M + m) * 2 + 1] = prv.im;
      }
    }
  }
  __syncthreads();
  double* d1 = ws + ws_steer1(B, S, F, M) + base * (M * 2);
  for (int i = tid; i < F * M * 2; i += blockDim.x) d1[i] = s_d[i];
  for (int f = tid; f < F; f += blockDim.x) {
    const double* pn = ws + ws_phin(B, S, F, M) + (base + f) * (M * M * 2);
    cd A[M][M + 1];
    PhinPrime P;
    if constexpr (EXT) P.init<M>(pn, cond, tn, epsi);
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if constexpr (EXT) {
#pragma unroll
        for (int j = 0; j < M; ++j) A[i][j] = P.at<M>(pn, i, j);
      } else {
#pragma unroll
      for (int j = 0; j < M; ++j) A[i][j] = {pn[(i * M + j) * 2], pn[(i * M + j) * 2 + 1]};
      A[i][i].re += epsi;                                 // tester.py:1086-1088,1221
      }
      A[i][M] = {s_d[(f * M + i) * 2], s_d[(f * M + i) * 2 + 1]};
    }
    // Gaussian elimination with partial pivoting (fully unrolled so A stays in registers)
#pragma unroll
    for (int k = 0; k < M; ++k) {
      int piv = k;
      double best = cabs2(A[k][k]);
#pragma unroll
      for (int i = k + 1; i < M; ++i) {
        const double v = cabs2(A[i][k]);
        if (v > best) { best = v; piv = i; }
      }
#pragma unroll
      for (int i = k + 1; i < M; ++i) {
        if (piv == i) {
#pragma unroll
          for (int j = 0; j <= M; ++j) { const cd tmp = A[k][j]; A[k][j] = A[i][j]; A[i][j] = tmp; }
        }
      }
      const cd pk = A[k][k];
#pragma unroll
      for (int i = k + 1; i < M; ++i) {
        const cd fac = cdiv(A[i][k], pk);
#pragma unroll
        for (int j = k; j <= M; ++j) A[i][j] = csub(A[i][j], cmul(fac, A[k][j]));
      }
    }
    cd x[M];
#pragma unroll
    for (int i = M - 1; i >= 0; --i) {
      cd acc = A[i][M];
#pragma unroll
      for (int j = i + 1; j < M; ++j) acc = csub(acc, cmul(A[i][j], x[j]));
      x[i] = cdiv(acc, A[i][i]);
    }
    cd den = {0.0, 0.0};                                  // d^H x (tester.py:1223)
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const cd di = {s_d[(f * M + i) * 2], s_d[(f * M + i) * 2 + 1]};
      den = cadd(den, cmul(cconj(di), x[i]));
    }
    double* wo = ws + ws_w(B, S, F, M) + (base + f) * (M * 2);
    if constexpr (EXT) {
#pragma unroll
      for (int i = 0; i < M; ++i) x[i] = cdiv(x[i], den);
      if (ban) ban_scale<M>(x, [&](int i, int j) { return P.at<M>(pn, i, j); });
#pragma unroll
      for (int i = 0; i < M; ++i) {
        wo[i * 2] = x[i].re;
        wo[i * 2 + 1] = x[i].im;
      }
    } else {
#pragma unroll
    for (int i = 0; i < M; ++i) {
      const cd wi = cdiv(x[i], den);
      wo[i * 2] = wi.re;
      wo[i * 2 + 1] = wi.im;
    }
    }
  }
