// Room simulator (include/misonet.h misonet_room_*): image-source room impulse responses of a shoebox in the
// Allen & Berkley (1979) family, and the scene mixer that convolves dry sources with them.  The project's own definition; nothing
// here was compared against pyroomacoustics, gpuRIR, rir_generator or sms_wsj.
//
//   N_i = ceil((Lh + W/2) c / (fs 2 L_i)),  images (n, q), n_i in [-N_i, N_i], q_i in {0, 1}, in the order n_x, n_y, n_z ascending,
//   then q = q_x q_y q_z from 000 to 111;  p_i = (1 - 2 q_i) s_i + 2 n_i L_i,  d = |p - r|,  tau = d fs / c,
//   g = prod_i beta_i0^|n_i - q_i| beta_i1^|n_i|,  rho = sum_i |n_i - q_i| + |n_i|;  kept: g > 0 and (max_order < 0 or rho <= max_order)
//   h[n] = sum over the kept images with |n - tau| < W/2 of  g / (4 pi d) * 1/2 (1 + cos(2 pi x / W)) * sinc(x),  x = n - tau
//
// room_rir_k is the gather form: one thread per output tap, every thread of a tile walks all images in the enumeration order and
// adds the ones that cover its tap, so the float64 sum has one fixed order without atomics and an output depends on nothing but
// its own pair of its own item.  The per-axis tables -- squared offset, gain and reflection count of each (n_i, q_i) -- sit in
// static LDS; an image is culled against the tile's delay window by d^2 before any square root (the cull is widened by 1e-9, the
// per-tap test |x| < W/2 is exact, so the cull changes no bit), and whole ranges of n_y and n_z are skipped analytically.
//
// room_mix_k: one thread per output sample of one (item, microphone), looping the sources; the taps (float64) and the input
// window (float32) of a chunk of RM_KC taps are staged in LDS, the sum is float64 FMAs with k ascending, `early` is the value of
// the same sum when k reaches the split, and images, early and mix are written in one pass.
#include "kernels.hpp"

#include <cmath>

namespace mn {

constexpr int RM_TILE = 256;             // taps (room_rir_k) and output samples (room_mix_k) per workgroup
constexpr int RM_KC = 512;               // taps per staged chunk of room_mix_k
constexpr int RM_ENT = 2 * (2 * ROOM_MAX_N + 1);   // table entries per axis
constexpr double RM_HALF = ROOM_W / 2.0;

int room_tile() { return RM_TILE; }

// b^k for 0 <= k <= 2 ROOM_MAX_N + 1 by squaring: at most 9 + 9 roundings, within 4e-15 of pow; b^0 = 1 for b = 0 too
__device__ __forceinline__ double rm_powi(double b, int k) {
  double r = 1.0;
#pragma unroll 1
  for (; k; k >>= 1) {
    if (k & 1) r *= b;
    b *= b;
  }
  return r;
}

// grid (B S M, ceil(Lh / RM_TILE)), RM_TILE threads
__global__ __launch_bounds__(RM_TILE) void room_rir_k(const double* __restrict__ room, const double* __restrict__ beta,
                                                      const double* __restrict__ src, const double* __restrict__ mic, int S, int M,
                                                      double fs, double c, int Lh, int max_order, double* __restrict__ rir,
                                                      int* __restrict__ fail) {
  __shared__ double s_d2[3][RM_ENT];     // squared offset along the axis of entry 2 (n + N) + q
  __shared__ double s_g[3][RM_ENT];      // its gain beta_0^|n - q| beta_1^|n|
  __shared__ unsigned short s_o[3][RM_ENT];   // its reflection count |n - q| + |n|
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int m = pair % M, s = (pair / M) % S, b = pair / (M * S);
  const int t0 = blockIdx.y * RM_TILE;
  const int tap = t0 + tid;
  double* out = rir + (long long)pair * Lh;

  // ---- arguments of this pair: every thread of every tile comes to the same verdict --------------------------------------
  int flag = 0, N0 = 0, N1 = 0, N2 = 0;
  double count = 8.0;
  bool wide = false;
#pragma unroll 1
  for (int i = 0; i < 3; ++i) {                                      // not unrolled: few values live at once
    const double Li = room[b * 3 + i], si = src[((long long)b * S + s) * 3 + i], ri = mic[((long long)b * M + m) * 3 + i];
    const double b0 = beta[b * 6 + 2 * i], b1 = beta[b * 6 + 2 * i + 1];
    if (!(Li > 0.0) || !isfinite(Li)) flag = 1;
    if (!(si >= 0.0 && si <= Li) || !(ri >= 0.0 && ri <= Li)) flag = 1;                     // a NaN fails both
    if (!(b0 >= 0.0 && b0 < 1.0) || !(b1 >= 0.0 && b1 < 1.0)) flag = 1;
    const double ni = ceil(((double)Lh + RM_HALF) * c / (fs * 2.0 * Li));
    int nn = 0;
    if (!(ni <= (double)ROOM_MAX_N)) wide = true;
    else nn = (int)ni;
    count *= 2.0 * ni + 1.0;
    if (i == 0) N0 = nn; else if (i == 1) N1 = nn; else N2 = nn;
  }
  if (!flag && (wide || !(count <= ROOM_MAX_IMAGES))) flag = 4;      // bit 0 wins: its N_i mean nothing
  if (flag) {                                                        // block-uniform
    if (tap < Lh) out[tap] = 0.0;
    if (blockIdx.y == 0 && tid == 0) fail[pair] = flag;
    return;
  }

  // ---- the tables ----------------------------------------------------------------------------------------------------------
#pragma unroll 1
  for (int i = 0; i < 3; ++i) {                                      // not unrolled: one copy of pow, the arguments read again
    const int Ni = i == 0 ? N0 : (i == 1 ? N1 : N2);
    const double Li = room[b * 3 + i], si = src[((long long)b * S + s) * 3 + i], ri = mic[((long long)b * M + m) * 3 + i];
    const double b0 = beta[b * 6 + 2 * i], b1 = beta[b * 6 + 2 * i + 1];
    for (int e = tid; e < 2 * (2 * Ni + 1); e += RM_TILE) {
      const int n = (e >> 1) - Ni, q = e & 1;
      const double off = (1.0 - 2.0 * q) * si + 2.0 * n * Li - ri;
      const int k0 = abs(n - q), k1 = abs(n);
      s_d2[i][e] = off * off;
      s_g[i][e] = rm_powi(b0, k0) * rm_powi(b1, k1);
      s_o[i][e] = (unsigned short)(k0 + k1);
    }
  }
  __syncthreads();

  // ---- the tile's window of squared distances: an image outside it covers no tap of this tile --------------------------------
  const int t1 = (t0 + RM_TILE < Lh ? t0 + RM_TILE : Lh) - 1;
  const double dlo = ((double)t0 - RM_HALF) * c / fs, dhi = ((double)t1 + RM_HALF) * c / fs;
  const double lo2 = dlo > 0.0 ? dlo * dlo * (1.0 - 1e-9) : -1.0;    // tile 0 keeps d = 0 (flag bit 1 is raised there)
  const double hi2 = dhi * dhi * (1.0 + 1e-9);
  const double two_lz = 2.0 * room[b * 3 + 2];
  const bool any_order = max_order < 0;
  const double pi = 3.14159265358979323846;
  const double tn = (double)tap;
  double h = 0.0;
  int near = 0;

  for (int nx = -N0; nx <= N0; ++nx) {
    const int ex = 2 * (nx + N0);
    const double x0 = s_d2[0][ex], x1 = s_d2[0][ex + 1];
    if ((x0 < x1 ? x0 : x1) >= hi2) continue;
    for (int ny = -N1; ny <= N1; ++ny) {
      const int ey = 2 * (ny + N1);
      const double y0 = s_d2[1][ey], y1 = s_d2[1][ey + 1];
      const double dmin = (x0 < x1 ? x0 : x1) + (y0 < y1 ? y0 : y1);
      if (dmin >= hi2) continue;
      // |p_z - r_z| lies in [2 (|n_z| - 1) L_z, 2 (|n_z| + 1) L_z]: beyond khi every image is past the window, up to klo before it
      const double dmax = (x0 < x1 ? x1 : x0) + (y0 < y1 ? y1 : y0);
      const double kh = floor(sqrt(hi2 - dmin) / two_lz) + 2.0;
      const int khi = kh < (double)N2 ? (int)kh : N2;
      int klo = -1;
      if (lo2 > dmax) klo = (int)floor(sqrt(lo2 - dmax) / two_lz) - 2;
      for (int nz = -khi; nz <= khi; ++nz) {
        if (nz >= -klo && nz <= klo) { nz = klo; continue; }        // skips [-klo, klo]; klo = -1: nothing
        const int ez = 2 * (nz + N2);
#pragma unroll 1
        for (int j = 0; j < 8; ++j) {                                // j = 4 q_x + 2 q_y + q_z: three loads, two adds, two compares
          const int jx = ex + (j >> 2), jy = ey + ((j >> 1) & 1), jz = ez + (j & 1);
          const double d2 = (s_d2[0][jx] + s_d2[1][jy]) + s_d2[2][jz];
          if (d2 >= hi2 || d2 <= lo2) continue;
          const double g = (s_g[0][jx] * s_g[1][jy]) * s_g[2][jz];
          if (!(g > 0.0)) continue;
          if (!any_order && (int)s_o[0][jx] + (int)s_o[1][jy] + (int)s_o[2][jz] > max_order) continue;
          const double d = sqrt(d2);
          if (d < 1e-3) { near = 2; continue; }
          const double x = tn - d * fs / c;
          if (fabs(x) < RM_HALF) {
            const double a = g / (4.0 * pi * d);
            const double px = pi * x;
            const double sinc = x == 0.0 ? 1.0 : sin(px) / px;
            h += a * (0.5 * (1.0 + cos(2.0 * pi * x / ROOM_W))) * sinc;
          }
        }
      }
    }
  }
  if (tap < Lh) out[tap] = h;
  if (blockIdx.y == 0 && tid == 0) fail[pair] = near;                // an image with d < 1e-3 has tau < 1: tile 0 sees it
}

// grid (ceil(Lo / RM_TILE), M, B), RM_TILE threads (the tiles of 2^24 samples do not fit grid.y)
__global__ __launch_bounds__(RM_TILE) void room_mix_k(const float* __restrict__ x, long long xsb, long long xss, long long xst,
                                                      const double* __restrict__ rir, const int* __restrict__ split, int S, int M,
                                                      int L, int Lh, int Lo, float* __restrict__ images,
                                                      float* __restrict__ early, float* __restrict__ mix) {
  __shared__ double s_h[RM_KC];
  __shared__ float s_x[RM_KC + RM_TILE];
  const int tid = threadIdx.x;
  const int m = blockIdx.y, b = blockIdx.z;
  const int n0 = blockIdx.x * RM_TILE;
  const int n = n0 + tid;
  const int kmax = n < Lh - 1 ? n : Lh - 1;                          // this output's last tap
  double total = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* h = rir + (((long long)b * S + s) * M + m) * Lh;
    const float* xs = x + (long long)b * xsb + (long long)s * xss;
    int sp = split ? split[b * S + s] : Lh;
    sp = sp < 0 ? 0 : sp;
    double acc = 0.0, acc_e = 0.0;
    bool taken = false;
    // the tile's outputs use taps 0 .. min(n0 + RM_TILE - 1, Lh - 1)
    const int kend = (n0 + RM_TILE - 1 < Lh - 1 ? n0 + RM_TILE - 1 : Lh - 1) + 1;
    for (int k0 = 0; k0 < kend; k0 += RM_KC) {
      const int kc = kend - k0 < RM_KC ? kend - k0 : RM_KC;
      const long long w0 = (long long)n0 - (k0 + kc - 1);            // the window's first input sample
      __syncthreads();
      for (int i = tid; i < kc; i += RM_TILE) s_h[i] = h[k0 + i];
      for (int i = tid; i < kc + RM_TILE - 1; i += RM_TILE) {
        const long long gi = w0 + i;
        s_x[i] = (gi >= 0 && gi < L) ? xs[gi * xst] : 0.0f;
      }
      __syncthreads();
      if (!taken && sp <= k0) { acc_e = acc; taken = true; }
      int je = kmax - k0 + 1;                                        // taps of this chunk that this output has
      je = je < kc ? je : kc;
      const float* xp = s_x + tid + kc - 1;                          // x[n - k0 - j] = xp[-j]
      int j = 0;
      if (!taken && sp < k0 + kc) {                                  // the split falls inside this chunk (block-uniform)
        const int js = sp - k0 < je ? sp - k0 : je;
        for (; j < js; ++j) acc = fma(s_h[j], (double)xp[-j], acc);
        acc_e = acc;
        taken = true;
      }
      for (; j < je; ++j) acc = fma(s_h[j], (double)xp[-j], acc);
    }
    if (!taken) acc_e = acc;                                         // split >= Lh: the same bits as the image
    if (n < Lo) {
      const long long at = ((((long long)b * S + s) * M + m) * Lo) + n;
      images[at] = (float)acc;
      if (early) early[at] = (float)acc_e;
    }
    total += acc;
  }
  if (mix && n < Lo) mix[((long long)b * M + m) * Lo + n] = (float)total;
}

hipError_t launch_room_rir(const double* room, const double* beta, const double* src, const double* mic, int B, int S, int M,
                           double fs, double c, int Lh, int max_order, double* rir, int* fail, hipStream_t s) {
  if (B < 1 || B > ROOM_MAX_B || S < 1 || S > ROOM_MAX_S || M < 1 || M > ROOM_MAX_M || Lh < 1 || Lh > ROOM_MAX_LH)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(B * S * M), (unsigned)((Lh + RM_TILE - 1) / RM_TILE));
  hipLaunchKernelGGL(room_rir_k, grid, dim3(RM_TILE), 0, s, room, beta, src, mic, S, M, fs, c, Lh, max_order, rir, fail);
  return hipGetLastError();
}

hipError_t launch_room_mix(const float* x, const long long* xs, const double* rir, const int* split, int B, int S, int M, int L,
                           int Lh, int Lo, float* images, float* early, float* mix, hipStream_t s) {
  if (B < 1 || B > ROOM_MAX_B || S < 1 || S > ROOM_MAX_S || M < 1 || M > ROOM_MAX_M || Lh < 1 || Lh > ROOM_MAX_LH || L < 1 ||
      L > ROOM_MAX_L || Lo < 1 || (long long)Lo > (long long)L + Lh - 1)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((Lo + RM_TILE - 1) / RM_TILE), (unsigned)M, (unsigned)B);
  if ((long long)grid.x * M * B * RM_TILE >= (1LL << 32)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(room_mix_k, grid, dim3(RM_TILE), 0, s, x, xs[0], xs[1], xs[2], rir, split, S, M, L, Lh, Lo, images, early, mix);
  return hipGetLastError();
}

}  // namespace mn
