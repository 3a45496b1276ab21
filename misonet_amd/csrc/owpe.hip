// Online WPE dereverberation (RLS-WPE: Yoshioka & Nakatani 2012; Caroselli et al. 2017) on the device: C ABI misonet_owpe* in
// api_array.hip; the definition is INTEGRATION.md 4r and is restated in NumPy in tests/owpe_ref.py.
//
// Per (item b, bin f), independent of every other, with N = M taps and R = delay + taps - 1.  The state of a bin is P [N][N]
// and G [N][M] complex128, the last R frames as the complex64 that was read, the powers of the last `context` frames, the frame
// count n, the ring position and the fail word.  Per new frame y, float64 after the load:
//
//   z[k M + m] = y[m, t - delay - k]                       from the frame ring
//   x = y - G^H z                                           the output, rounded to complex64 once
//   lambda = max(mean of p over the min(n, context) + 1 latest frames, power_floor),  p = mean_m |y_m|^2
//   u = P z,  d = alpha lambda + Re(z^H u),  k = u / d
//   P <- (P - k u^H) / alpha                               lower triangle computed, upper triangle its mirror: exactly Hermitian
//   G <- G + k x^H
//
//   owpe_reset_k  P = init I, everything else 0 (behind one memset of the state)
//   owpe_k        one workgroup of 8 waves per bin walks the T frames of the call in order.  P (odd row pitch: the mirror stores
//                 of a column land on different banks), G transposed, the frame ring and the power ring are loaded into LDS once
//                 and written back once.  Per frame, three barriers:
//                   1. thread m takes the frame it loaded one frame ahead, z is built from the ring;
//                   2. wave w owns the rows w, w + 8, ... of u = P z: lane l multiplies the columns l and l + 64, a butterfly adds
//                      the 64 lanes; wave m also forms x[m] the same way;
//                   3. every wave forms d with the same butterfly (the same bits on every thread, no broadcast), then the
//                      triangle of P, G, the output, the rings.
//
// Every sum has one fixed order that depends on nothing but N and M, nothing is accumulated with atomics and a bin never looks
// at another one: the result is bit-reproducible, does not depend on the batch or the position in it, and -- the state being all
// that passes from one frame to the next -- does not depend on how the stream is cut into calls.  One launch, no host
// synchronisation, no allocation.
//
// A failing frame (a non-finite sample, or d not finite or not > 0) is passed through: x = y, P and G stay, zeros enter both
// rings, fail |= 1, n advances.
#include "kernels.hpp"
#include "cplx.hpp"

namespace mn {

constexpr int OWPE_THREADS = 512, OWPE_WAVES = OWPE_THREADS / 64;

// state: fail int [bins] | n int [bins] | pos int [bins] | pw f64 [bins][CTX] | ring c64 [bins][R][M] | G c128 [bins][N][M] |
//        P c128 [bins][N][N]
struct OwpeWs { long long fail, n, pos, pw, ring, g, p, total; };
__host__ __device__ inline OwpeWs owpe_ws(long long bins, int M, int taps, int delay) {
  const long long N = (long long)M * taps, R = (long long)delay + taps - 1;
  OwpeWs w;
  w.fail = 0;
  w.n = align16(bins * 4);
  w.pos = align16(w.n + bins * 4);
  w.pw = align16(w.pos + bins * 4);
  w.ring = align16(w.pw + bins * OWPE_CTX * 8);
  w.g = align16(w.ring + bins * R * M * 8);
  w.p = align16(w.g + bins * N * M * 16);
  w.total = align16(w.p + bins * N * N * 16);
  return w;
}
long long owpe_state_bytes(long long bins, int M, int taps, int delay) { return owpe_ws(bins, M, taps, delay).total; }

// LDS of owpe_k: the vectors of one frame are static (OwpeFrame below), the state is the dynamic block, in bytes from its start
constexpr int OWPE_NMAX = 80, OWPE_MMAX = 8;
struct OwpeFrame {
  double2 u[OWPE_NMAX], z[OWPE_NMAX], x[OWPE_MMAX], y[OWPE_MMAX];
  double pw[2][OWPE_CTX];                                              // read from one, shifted into the other
  int bad[OWPE_MMAX];
  double par[3];                                                       // alpha, 1 / alpha, power_floor: read per frame, not held in SGPRs
};
struct OwpeLds { int P, G, ring, total, np; };
__host__ __device__ inline OwpeLds owpe_lds(int M, int taps, long long delay) {
  const int N = M * taps;
  const long long R = delay + taps - 1;
  OwpeLds l;
  l.np = N | 1;                                                        // double2 per row of P
  l.P = 0;                                                             // double2 [N][np]
  l.G = l.P + N * l.np * 16;                                           // double2 [M][N]: G transposed
  l.ring = l.G + M * N * 16;                                           // float2 [R][M]
  const long long tot = l.ring + R * M * 8 + (long long)sizeof(OwpeFrame);
  l.total = tot > (1LL << 30) ? (1 << 30) : (int)tot;                  // with the static part: what the workgroup takes
  return l;
}
long long owpe_lds_bytes(int M, int taps, int delay) { return owpe_lds(M, taps, delay).total; }

struct OwpeArgs {
  const float2* mix;
  float2* out;
  char* state;
  OwpeWs w;
  int M, T, F, taps, delay, context;
  double alpha, inv_alpha, power_floor;
};

// the state of one bin
struct OwpeState { int *fail, *n, *pos; double* pw; float2* ring; double2 *g, *p; };
__device__ __forceinline__ OwpeState owpe_state(const OwpeArgs& a, long long bin, int N, int R) {
  OwpeState s;
  s.fail = reinterpret_cast<int*>(a.state + a.w.fail) + bin;
  s.n = reinterpret_cast<int*>(a.state + a.w.n) + bin;
  s.pos = reinterpret_cast<int*>(a.state + a.w.pos) + bin;
  s.pw = reinterpret_cast<double*>(a.state + a.w.pw) + bin * OWPE_CTX;
  s.ring = reinterpret_cast<float2*>(a.state + a.w.ring) + bin * R * a.M;
  s.g = reinterpret_cast<double2*>(a.state + a.w.g) + bin * N * a.M;
  s.p = reinterpret_cast<double2*>(a.state + a.w.p) + bin * N * N;
  return s;
}

// P [N][N] -> LDS rows of pitch np, G [N][M] -> Gt [M][N], the rings as they are; and back
__device__ __forceinline__ void owpe_load(const OwpeState& s, int N, int M, int R, int np, double2* P, double2* Gt, float2* ring,
                                          double* pw) {
  const int tid = threadIdx.x;
  for (int e = tid; e < N * N; e += OWPE_THREADS) {
    const int i = e / N, j = e - i * N;
    P[i * np + j] = s.p[e];
  }
  for (int e = tid; e < N * M; e += OWPE_THREADS) {
    const int m = e / N, j = e - m * N;
    Gt[e] = s.g[j * M + m];
  }
  for (int e = tid; e < R * M; e += OWPE_THREADS) ring[e] = s.ring[e];
  if (tid < OWPE_CTX) pw[tid] = s.pw[tid];
}
__device__ __forceinline__ void owpe_store(const OwpeState& s, int N, int M, int R, int np, const double2* P, const double2* Gt,
                                           const float2* ring, const double* pw) {
  const int tid = threadIdx.x;
  for (int e = tid; e < N * N; e += OWPE_THREADS) {
    const int i = e / N, j = e - i * N;
    s.p[e] = P[i * np + j];
  }
  for (int e = tid; e < N * M; e += OWPE_THREADS) {
    const int m = e / N, j = e - m * N;
    s.g[j * M + m] = Gt[e];
  }
  for (int e = tid; e < R * M; e += OWPE_THREADS) s.ring[e] = ring[e];
  if (tid < OWPE_CTX) s.pw[tid] = pw[tid];
}

// grid (bins), 64 threads: P = init I behind the memset
__global__ __launch_bounds__(64) void owpe_reset_k(char* state, long long bins, int M, int taps, int delay, double init) {
  const OwpeWs w = owpe_ws(bins, M, taps, delay);
  const int N = M * taps;
  double2* P = reinterpret_cast<double2*>(state + w.p) + (long long)blockIdx.x * N * N;
  for (int i = threadIdx.x; i < N; i += 64) P[(long long)i * N + i] = make_double2(init, 0.0);
}

// grid (bins), 512 threads, owpe_lds(M, taps, delay).total - sizeof(OwpeFrame) bytes of dynamic LDS
__global__ __launch_bounds__(OWPE_THREADS) void owpe_k(const OwpeArgs a) {
  extern __shared__ __align__(16) unsigned char owpe_smem[];
  const int M = a.M, T = a.T, F = a.F, taps = a.taps, N = M * taps, R = a.delay + taps - 1;
  const OwpeLds l = owpe_lds(M, taps, a.delay);
  const int np = l.np;
  double2* P = reinterpret_cast<double2*>(owpe_smem + l.P);
  double2* Gt = reinterpret_cast<double2*>(owpe_smem + l.G);
  __shared__ OwpeFrame fr;
  double2 *ul = fr.u, *zl = fr.z, *xl = fr.x, *yl = fr.y;
  double* pwl = fr.pw[0];
  int* badl = fr.bad;
  float2* ring = reinterpret_cast<float2*>(owpe_smem + l.ring);

  const long long bin = blockIdx.x;
  const int b = (int)(bin / F), f = (int)(bin - (long long)b * F);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // frame t of microphone m: mix[((b M + m) T + t) F + f]
  const float2* src = a.mix + ((long long)b * M + (tid < M ? tid : 0)) * T * F + f;
  float2* dst = a.out + ((long long)b * M + (tid < M ? tid : 0)) * T * F + f;

  // ---- the state into LDS
  int n, pos, failw, cur = 0;                                          // uniform over the workgroup
  {
    const OwpeState st = owpe_state(a, bin, N, R);
    owpe_load(st, N, M, R, np, P, Gt, ring, pwl);
    n = *st.n; pos = *st.pos; failw = *st.fail;
    if ((unsigned)pos >= (unsigned)R) pos = 0;                         // a state that was never reset must not index past the ring
  }

  if (tid == 0) { fr.par[0] = a.alpha; fr.par[1] = a.inv_alpha; fr.par[2] = a.power_floor; }
  float2 ynext = make_float2(0.f, 0.f);
  if (tid < M) ynext = *src;

#pragma unroll 1
  for (int t = 0; t < T; ++t) {
    // ---- 1. the frame and its stacked past
    __syncthreads();
    const float2 yraw = ynext;
    if (tid < M) {
      yl[tid] = make_double2((double)yraw.x, (double)yraw.y);
      badl[tid] = !(finite(yraw.x) && finite(yraw.y));
      src += F;
      if (t + 1 < T) ynext = *src;
    }
    for (int e = tid; e < N; e += OWPE_THREADS) {
      const int k = e / M, m = e - k * M;
      int slot = pos - a.delay - k;                                    // the frame a = delay + k back, 1 <= a <= R
      if (slot < 0) slot += R;
      const float2 v = ring[slot * M + m];
      zl[e] = make_double2((double)v.x, (double)v.y);
    }
    __syncthreads();

    // ---- 2. u = P z by rows, x = y - G^H z
    {
      const int j0 = lane, j1 = lane + 64;
      double2 z0 = make_double2(0.0, 0.0), z1 = z0;
      if (j0 < N) z0 = zl[j0];
      if (j1 < N) z1 = zl[j1];
      for (int i = wave; i < N; i += OWPE_WAVES) {
        double sr = 0.0, si = 0.0;
        if (j0 < N) {
          const double2 p = P[i * np + j0];
          sr = p.x * z0.x - p.y * z0.y;
          si = p.x * z0.y + p.y * z0.x;
        }
        if (j1 < N) {
          const double2 p = P[i * np + j1];
          sr += p.x * z1.x - p.y * z1.y;
          si += p.x * z1.y + p.y * z1.x;
        }
        sr = wave_sum(sr);
        si = wave_sum(si);
        if (lane == 0) ul[i] = make_double2(sr, si);
      }
      if (wave < M) {                                                  // conj(G[j][m]) z[j]
        double sr = 0.0, si = 0.0;
        if (j0 < N) {
          const double2 g = Gt[wave * N + j0];
          sr = g.x * z0.x + g.y * z0.y;
          si = g.x * z0.y - g.y * z0.x;
        }
        if (j1 < N) {
          const double2 g = Gt[wave * N + j1];
          sr += g.x * z1.x + g.y * z1.y;
          si += g.x * z1.y - g.y * z1.x;
        }
        sr = wave_sum(sr);
        si = wave_sum(si);
        if (lane == 0) {
          const double2 y = yl[wave];
          xl[wave] = make_double2(y.x - sr, y.y - si);
        }
      }
      __syncthreads();

      // ---- 3. d on every thread, then the updates
      double zu = 0.0;
      if (j0 < N) { const double2 u = ul[j0]; zu = z0.x * u.x + z0.y * u.y; }
      if (j1 < N) { const double2 u = ul[j1]; zu += z1.x * u.x + z1.y * u.y; }
      zu = wave_sum(zu);
      int bad = 0;
      double p = 0.0;
#pragma unroll 1
      for (int m = 0; m < M; ++m) {                                    // fixed order: microphone 0, 1, ...
        const double2 y = yl[m];
        p += y.x * y.x + y.y * y.y;
        bad |= badl[m];
      }
      p /= (double)M;
      const double* pw = pwl + cur * OWPE_CTX;
      const int cnt = n < a.context ? n : a.context;
      double lam = p;
#pragma unroll 1
      for (int c = 0; c < cnt; ++c) lam += pw[c];                      // the latest first
      const double alpha = fr.par[0], inv_alpha = fr.par[1];
      lam = fmax(lam / (double)(cnt + 1), fr.par[2]);
      const double d = alpha * lam + zu;
      const bool failed = bad || !(d > 0.0 && d <= F64_MAX);

      if (!failed) {
        const double invd = 1.0 / d;
        // the lower triangle, rows r and N - 1 - r folded into one strip of N + 1 elements; the mirror is its conjugate
        const int H = (N + 1) >> 1;
        for (int e = tid; e < H * (N + 1); e += OWPE_THREADS) {
          const int r = e / (N + 1), c = e - r * (N + 1);
          int i, j;
          if (c <= r) { i = r; j = c; }
          else { i = N - 1 - r; j = c - r - 1; if (i == r) continue; }
          const double2 ui = ul[i], uj = ul[j], pij = P[i * np + j];
          double2 v;
          v.x = (pij.x - (ui.x * uj.x + ui.y * uj.y) * invd) * inv_alpha;
          v.y = (pij.y - (ui.y * uj.x - ui.x * uj.y) * invd) * inv_alpha;
          if (i == j) v.y = 0.0;
          P[i * np + j] = v;
          if (i != j) P[j * np + i] = make_double2(v.x, -v.y);
        }
        for (int e = tid; e < M * N; e += OWPE_THREADS) {              // G[j][m] += k[j] conj(x[m])
          const int m = e / N, j = e - m * N;
          const double2 u = ul[j], x = xl[m];
          const double kr = u.x * invd, ki = u.y * invd;
          double2 g = Gt[e];
          g.x += kr * x.x + ki * x.y;
          g.y += ki * x.x - kr * x.y;
          Gt[e] = g;
        }
      }
      if (tid < M) {
        const double2 x = xl[tid];
        *dst = failed ? yraw : make_float2((float)x.x, (float)x.y);
        dst += F;
        ring[pos * M + tid] = failed ? make_float2(0.f, 0.f) : yraw;
      }
      if (tid < OWPE_CTX) pwl[(cur ^ 1) * OWPE_CTX + tid] = tid == 0 ? (failed ? 0.0 : p) : pw[tid - 1];
      if (failed) failw |= 1;
    }
    cur ^= 1;
    pos = pos + 1 == R ? 0 : pos + 1;
    if (n < 0x7fffffff) ++n;
  }
  __syncthreads();

  // ---- the state back
  const OwpeState st = owpe_state(a, bin, N, R);
  owpe_store(st, N, M, R, np, P, Gt, ring, pwl + cur * OWPE_CTX);
  if (tid == 0) { *st.n = n; *st.pos = pos; *st.fail = failw; }
}

hipError_t owpe_init() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&owpe_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                             OWPE_LDS_LIMIT - (int)sizeof(OwpeFrame));
}

hipError_t launch_owpe_reset(void* state, int B, int M, int F, int taps, int delay, double init, hipStream_t s) {
  const long long bins = (long long)B * F;
  hipError_t e = hipMemsetAsync(state, 0, owpe_state_bytes(bins, M, taps, delay), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(owpe_reset_k, dim3((unsigned)bins), dim3(64), 0, s, reinterpret_cast<char*>(state), bins, M, taps, delay, init);
  return hipGetLastError();
}

hipError_t launch_owpe(const void* mix, int B, int M, int T, int F, int taps, int delay, int context, double alpha,
                       double power_floor, void* out, void* state, hipStream_t s) {
  const int lds = owpe_lds(M, taps, delay).total - (int)sizeof(OwpeFrame);
  if (lds + (int)sizeof(OwpeFrame) > OWPE_LDS_LIMIT) return hipErrorInvalidValue;
  OwpeArgs a;
  a.mix = reinterpret_cast<const float2*>(mix);
  a.out = reinterpret_cast<float2*>(out);
  a.state = reinterpret_cast<char*>(state);
  a.w = owpe_ws((long long)B * F, M, taps, delay);
  a.M = M; a.T = T; a.F = F; a.taps = taps; a.delay = delay; a.context = context;
  a.alpha = alpha; a.inv_alpha = 1.0 / alpha; a.power_floor = power_floor;
  hipLaunchKernelGGL(owpe_k, dim3((unsigned)((long long)B * F)), dim3(OWPE_THREADS), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_owpe_debug(const void* state, int B, int M, int F, int taps, int delay, void* g, void* p, int* fail, int* n,
                             hipStream_t s) {
  const long long bins = (long long)B * F, N = (long long)M * taps;
  const OwpeWs w = owpe_ws(bins, M, taps, delay);
  return copy_parts(state, {{g, w.g, bins * N * M * 16}, {p, w.p, bins * N * N * 16}, {fail, w.fail, bins * 4}, {n, w.n, bins * 4}},
                    s);
}

}  // namespace mn
