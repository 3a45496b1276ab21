// The body of mvdr_scm_eig<M> and of bf_scm<M> (mvdr.hip includes it into both, so that the kernel of the
// reference's live path compiles from the same text whatever the other one needs).  In scope: M, MIX, a, ws.
  constexpr int NT = M * (M + 1) / 2;
  __shared__ double s_part[4][2 * NT * 2];
  __shared__ double s_A[M][M][2];
  __shared__ double s_V[M][M][2];
  const int f = blockIdx.x, b = blockIdx.y, spk = blockIdx.z;
  const int tid = threadIdx.x;
  const float *sre[M], *sim[M], *yre[M], *yim[M];
  int sst = 1;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    src_row(a, b, f, m, spk, sre[m], sim[m], sst);
    const long long off = (long long)b * a.mix.sb + (long long)f * a.mix.sf + (long long)m * a.mix.sm;
    yre[m] = a.mix.re + off;
    yim[m] = a.mix.im + off;
  }
  const int yst = a.mix.st;
  float ps[NT][2], pn[NT][2];
#pragma unroll
  for (int i = 0; i < NT; ++i) { ps[i][0] = ps[i][1] = pn[i][0] = pn[i][1] = 0.f; }
  const int nthr = blockDim.x, nw = nthr >> 6;
  for (int t = tid; t < a.T; t += nthr) {
    float xr[M], xi[M], nr[M], ni[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      xr[m] = sre[m][(long long)t * sst];
      xi[m] = sim[m][(long long)t * sst];
      if constexpr (MIX) {
        nr[m] = yre[m][(long long)t * yst];              // noise = mix (tester.py:1096)
        ni[m] = yim[m][(long long)t * yst];
      } else {
        nr[m] = yre[m][(long long)t * yst] - xr[m];      // noise = mix - source (tester.py:1095)
        ni[m] = yim[m][(long long)t * yst] - xi[m];
      }
    }
    int k = 0;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j, ++k) {
        ps[k][0] += xr[i] * xr[j] + xi[i] * xi[j];
        ps[k][1] += xi[i] * xr[j] - xr[i] * xi[j];
        pn[k][0] += nr[i] * nr[j] + ni[i] * ni[j];
        pn[k][1] += ni[i] * nr[j] - nr[i] * ni[j];
      }
  }
  // block reduction in float64
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < NT; ++k)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      double v1 = ps[k][c], v2 = pn[k][c];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) {
        v1 += __shfl_xor(v1, m, 64);
        v2 += __shfl_xor(v2, m, 64);
      }
      if (lane == 0) {
        s_part[wave][(k * 2 + c)] = v1;
        s_part[wave][2 * NT + (k * 2 + c)] = v2;
      }
    }
  __syncthreads();
  const double invT = 1.0 / (double)a.T;
  const long long idx = ((long long)(b * a.S + spk) * a.F + f);
  for (int e = tid; e < 2 * NT * 2; e += nthr) {
    double v = 0.0;
    for (int w = 0; w < nw; ++w) v += s_part[w][e];
    v *= invT;
    const int which = e / (2 * NT);            // 0: Phi_s, 1: Phi_n
    const int kc = e - which * 2 * NT;
    const int k = kc >> 1, c = kc & 1;
    // k -> (i, j), i >= j
    int i = 0, rem = k;
    while (rem > i) { rem -= (i + 1); ++i; }
    const int j = rem;
    if (which == 0 && a.kind != BF_MVDR) {       // souden, gev: Phi_s beside Phi_n, the eigen-solve is bf_solve's
      double* ps_o = ws + ws_phis(a.B, a.S, a.F, M) + idx * (M * M * 2);
      ps_o[(i * M + j) * 2 + c] = (i == j && c) ? 0.0 : v;
      if (i != j) ps_o[(j * M + i) * 2 + c] = c ? -v : v;
    } else if (which == 0) {
      s_A[i][j][c] = v;
      s_A[j][i][c] = c ? -v : v;
      if (i == j && c) s_A[i][i][1] = 0.0;
    } else {
      double* pn_o = ws + ws_phin(a.B, a.S, a.F, M) + idx * (M * M * 2);
      pn_o[(i * M + j) * 2 + c] = (i == j && c) ? 0.0 : v;
      if (i != j) pn_o[(j * M + i) * 2 + c] = c ? -v : v;
    }
  }
  if (a.kind != BF_MVDR) return;                // uniform
  for (int e = tid; e < M * M; e += nthr) {
    const int i = e / M, j = e - i * M;
    s_V[i][j][0] = (i == j) ? 1.0 : 0.0;
    s_V[i][j][1] = 0.0;
  }
  __syncthreads();
  jacobi_hermitian<M>(s_A, s_V, tid);
  if (tid == 0) {
    int best = 0;                                         // argmax eigenvalue, first on ties (tester.py:1110)
    for (int i = 1; i < M; ++i)
      if (s_A[i][i][0] > s_A[best][best][0]) best = i;
    cd v[M];
    for (int i = 0; i < M; ++i) v[i] = {s_V[i][best][0], s_V[i][best][1]};
    const cd v0 = v[0];
    double nrm = 0.0;
    for (int i = 0; i < M; ++i) {
      v[i] = cdiv(v[i], v0);                              // tester.py:1119
      nrm += cabs2(v[i]);
    }
    const double sc = sqrt((double)M / sqrt(nrm));        // tester.py:1123: sqrt(M / ||d||)
    double* o = ws + ws_steer0(a.B, a.S, a.F, M) + idx * (M * 2);
    for (int i = 0; i < M; ++i) {
      o[i * 2 + 0] = v[i].re * sc;
      o[i * 2 + 1] = v[i].im * sc;
    }
  }
