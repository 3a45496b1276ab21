// STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) on the device (C ABI misonet_stoi_resample / misonet_stoi_measure in
// net.hip; the definition is INTEGRATION.md 4f, restated in NumPy in tests/stoi_ref.py; the dataclass is formed in score.py).
//
//   stoi_resample_k  x10[item][signal][m] = sum_j x[j] g[m q - j p + Lh], j ascending: the polyphase resampler to 10 kHz over
//                    the strided views of misonet_score_wave (references, estimates, the mixture), every signal once
//   stoi_energy_k    e[item][reference][frame] = 20 log10(|w frame| + EPS), one wave per frame
//   stoi_mask_k      per reference: the largest e, the mask e > max - 40 and, by an exclusive count, the list of kept frames;
//                    K stays in device memory (meta), the grids of the next kernels are sized by all frames
//   stoi_band_k      one workgroup per (new frame, signal, mask): the frame from its three kept neighbours (what overlap-add
//                    and framing again give, without the signal in between), the 512-point transform in LDS, 15 band sums
//   stoi_seg_k       one wave per segment of 30 frames: the clipped row correlations (STOI) and the row / column normalised
//                    correlation (ESTOI) of every (estimate, reference) pair
//   stoi_fold_k      the segments added in a fixed order, divided by 15 M and 30 M
//
// float64 throughout, no atomics, every sum in a fixed order, and an item never looks at another one: a result is
// bit-reproducible and does not depend on the batch it sits in or on its position there.
#include "kernels.hpp"

#include <cmath>
#include <vector>

namespace mn {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_J = 15, ST_NSEG = 30;
constexpr double ST_EPS = 0x1p-52;
constexpr double ST_CLIP = 1.0 + 5.623413251903491;     // 1 + 10^(15 / 20)
constexpr double ST_SHORT = 1e-5;                       // fewer than 30 kept frames
// the table: window [256], twiddles (cos, sin)(2 pi k / 512) [256][2], then the taps of 16 kHz, 8 kHz and 10 kHz
constexpr int ST_T_WIN = 0, ST_T_TW = 256, ST_T_TAPS = 768;

__constant__ int ST_LO[ST_J] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int ST_HI[ST_J] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// ---- host: the rates and the table ---------------------------------------------------------------------------------------
// p / q = 10000 / fs reduced, fc = 1 / (2 max(p, q)), Lh = ceil((60 - 8) / (28.714 fc / 10)); off = where the 2 Lh + 1 taps of
// the rate start in the table (16 kHz, then 8 kHz, then the single tap of 10 kHz)
static int stoi_half_len(int p, int q) {
  if (p == q) return 0;
  const double fc = 1.0 / (2.0 * (p > q ? p : q));
  return (int)std::ceil((60.0 - 8.0) / (28.714 * fc / 10.0));
}
static bool stoi_rate(int fs, int* p, int* q, int* Lh, int* off) {
  const int L16 = stoi_half_len(5, 8), L8 = stoi_half_len(5, 4);
  if (fs == 16000) { *p = 5; *q = 8; *Lh = L16; *off = ST_T_TAPS; return true; }
  if (fs == 8000) { *p = 5; *q = 4; *Lh = L8; *off = ST_T_TAPS + 2 * L16 + 1; return true; }
  if (fs == 10000) { *p = 1; *q = 1; *Lh = 0; *off = ST_T_TAPS + 2 * L16 + 1 + 2 * L8 + 1; return true; }
  return false;
}

int stoi_table_count() {
  int p, q, Lh, off;
  stoi_rate(10000, &p, &q, &Lh, &off);
  return off + 1;
}

int stoi_tap_offset(int fs) {
  int p, q, Lh, off;
  return stoi_rate(fs, &p, &q, &Lh, &off) ? off : -1;
}

long long stoi_resampled_len(long long n, int fs) {
  int p, q, Lh, off;
  if (!stoi_rate(fs, &p, &q, &Lh, &off) || n < 1 || n > (1LL << 24)) return -1;
  return (n * p + q - 1) / q;
}

int stoi_taps(int fs) {
  int p, q, Lh, off;
  return stoi_rate(fs, &p, &q, &Lh, &off) ? 2 * Lh + 1 : -1;
}

void stoi_build_table(double* t) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < ST_FRAME; ++k) t[ST_T_WIN + k] = 0.5 - 0.5 * std::cos(2.0 * pi * (k + 1) / (ST_FRAME + 1));
  for (int k = 0; k < ST_NFFT / 2; ++k) {
    t[ST_T_TW + 2 * k] = std::cos(2.0 * pi * k / ST_NFFT);
    t[ST_T_TW + 2 * k + 1] = std::sin(2.0 * pi * k / ST_NFFT);
  }
  const int rates[2] = {16000, 8000};
  for (int r = 0; r < 2; ++r) {
    int p, q, Lh, off;
    stoi_rate(rates[r], &p, &q, &Lh, &off);
    const double fc = 1.0 / (2.0 * (p > q ? p : q)), beta = 0.1102 * (60.0 - 8.7);
    std::vector<double> h(2 * Lh + 1);
    double sum = 0.0;
    for (int i = -Lh; i <= Lh; ++i) {
      const double a = pi * 2.0 * fc * i;
      const double sinc = i == 0 ? 1.0 : std::sin(a) / a;
      const double u = (double)i / Lh;
      const double kaiser = sig_i0(beta * std::sqrt(1.0 - u * u)) / sig_i0(beta);
      h[i + Lh] = 2.0 * p * fc * sinc * kaiser;
      sum += h[i + Lh];
    }
    for (int i = 0; i <= 2 * Lh; ++i) t[off + i] = p * h[i] / sum;
  }
  t[stoi_tap_offset(10000)] = 1.0;
}

// ---- the resampler -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long stoi_len10(long long nv, int p, int q) { return (nv * p + q - 1) / q; }

// grid (ceil(n10 / 256), NS signals, items), 256 threads over the output samples.  Signal s < R: reference s; s < R + E:
// estimate s - R; else the mixture.  Samples past the item's own length are written as zeros.
__global__ __launch_bounds__(256) void stoi_resample_k(const SigView ref, const SigView est, const SigView mix, int R, int E,
                                                       long long n, const int* n_valid, int p, int q, int Lh, const double* g,
                                                       long long n10, double* x10, int* len10) {
  const int s = blockIdx.y, b = blockIdx.z, NS = gridDim.y;
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nv = sig_nv(n_valid, b, n);
  const long long l10 = stoi_len10(nv, p, q);
  if (m == 0 && s == 0) len10[b] = (int)l10;
  if (m >= n10) return;
  long long base;
  const SigView& v = sig_pick(ref, est, mix, R, E, s, b, &base);
  double acc = 0.0;
  if (m < l10) {
    const long long c = m * q;
    long long j_lo = c - Lh <= 0 ? 0 : (c - Lh + p - 1) / p;          // ceil((m q - Lh) / p), not below 0
    long long j_hi = (c + Lh) / p;                                    // floor((m q + Lh) / p), not above nv - 1
    if (j_hi > nv - 1) j_hi = nv - 1;
    if (v.i16) {
      const int16_t* x = reinterpret_cast<const int16_t*>(v.p) + base;
      for (long long j = j_lo; j <= j_hi; ++j) acc += (double)x[j * v.st] * g[c - j * p + Lh];
      acc *= SIG_I16_UNIT;                                            // scaled once, after the sum
    } else {
      const float* x = reinterpret_cast<const float*>(v.p) + base;
      for (long long j = j_lo; j <= j_hi; ++j) acc += (double)x[j * v.st] * g[c - j * p + Lh];
    }
  }
  x10[((long long)b * NS + s) * n10 + m] = acc;
}

hipError_t launch_stoi_resample(const SigView& est, const SigView& ref, const SigView& mix, int B, int E, int R, long long n,
                                const int* n_valid, int fs, const double* table, double* x10, int* len10, hipStream_t s) {
  int p, q, Lh, off;
  if (!stoi_rate(fs, &p, &q, &Lh, &off)) return hipErrorInvalidValue;
  const long long n10 = (n * p + q - 1) / q;
  const int NS = R + E + (mix.p ? 1 : 0);
  hipLaunchKernelGGL(stoi_resample_k, dim3((unsigned)((n10 + 255) / 256), NS, B), dim3(256), 0, s, ref, est, mix, R, E, n,
                     n_valid, p, q, Lh, table + off, n10, x10, len10);
  return hipGetLastError();
}

// ---- frames, mask, bands, segments -------------------------------------------------------------------------------------
__host__ __device__ inline long long stoi_frames(long long len) { return len >= ST_FRAME ? (len - ST_FRAME) / ST_HOP + 1 : 0; }

// scratch of one item, in doubles: e [R][nf], tob [R][1 + NE][15][nf], part [R][NE][M][2], idx (int) [R][nf]
struct StoiLay { long long nf, M, e, tob, part, idx, total; };
__host__ __device__ inline StoiLay stoi_layout(int NS, int R, long long n10) {
  StoiLay L;
  const long long f = stoi_frames(n10), NE = NS - R;
  L.nf = f > 0 ? f : 1;
  L.M = f >= ST_NSEG ? f - ST_NSEG + 1 : 1;
  L.e = 0;
  L.tob = L.e + R * L.nf;
  L.part = L.tob + R * (1 + NE) * ST_J * L.nf;
  L.idx = L.part + R * NE * L.M * 2;
  L.total = L.idx + R * ((L.nf + 1) / 2);
  return L;
}
long long stoi_item_doubles(int NS, int R, long long n10) { return stoi_layout(NS, R, n10).total; }

// grid (ceil(nf / 4), R, items), 256 threads: wave w takes frame 4 x + w.  Lane l adds the squares of samples l, l + 64,
// l + 128, l + 192 in that order; 64-lane butterfly.
__global__ __launch_bounds__(256) void stoi_energy_k(const double* x10, const int* len10, int NS, int R, long long n10,
                                                     const double* table, double* scratch) {
  const int r = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const StoiLay L = stoi_layout(NS, R, n10);
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= stoi_frames(sig_nv(len10, b, n10))) return;
  const double* x = x10 + ((long long)b * NS + r) * n10 + i * ST_HOP;
  const double* w = table + ST_T_WIN;
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = w[lane + 64 * k] * x[lane + 64 * k];
    v += a * a;
  }
#pragma unroll
  for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  if (lane == 0) scratch[(long long)b * L.total + L.e + (long long)r * L.nf + i] = 20.0 * log10(sqrt(v) + ST_EPS);
}

// grid (R, items), 256 threads.  Thread t owns the frames [t c, t c + c), c = ceil(frames / 256): it counts its kept frames,
// the counts of the threads before it give its place in the list.  meta[item][reference] = (frames, kept, any sample != 0).
__global__ __launch_bounds__(256) void stoi_mask_k(const double* x10, const int* len10, int NS, int R, long long n10,
                                                   double* scratch, int* meta) {
  __shared__ double s_max[256];
  __shared__ int s_cnt[256];
  __shared__ int s_nz[256];
  const int r = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const StoiLay L = stoi_layout(NS, R, n10);
  const long long len = sig_nv(len10, b, n10), nf = stoi_frames(len);
  const double* e = scratch + (long long)b * L.total + L.e + (long long)r * L.nf;
  int* idx = reinterpret_cast<int*>(scratch + (long long)b * L.total + L.idx) + (long long)r * L.nf;
  const double* x = x10 + ((long long)b * NS + r) * n10;
  double mx = -1.0e308;
  for (long long i = t; i < nf; i += 256) mx = e[i] > mx ? e[i] : mx;
  int nz = 0;
  for (long long i = t; i < len; i += 256) nz |= x[i] != 0.0;
  s_max[t] = mx;
  s_nz[t] = nz;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (t < k) {
      s_max[t] = s_max[t + k] > s_max[t] ? s_max[t + k] : s_max[t];
      s_nz[t] |= s_nz[t + k];
    }
    __syncthreads();
  }
  const double thr = s_max[0] - 40.0;
  const long long c = (nf + 255) / 256;
  const long long lo = t * c < nf ? t * c : nf, hi = lo + c < nf ? lo + c : nf;
  int cnt = 0;
  for (long long i = lo; i < hi; ++i) cnt += e[i] > thr;
  s_cnt[t] = cnt;
  __syncthreads();
  int at = 0;
  for (int k = 0; k < t; ++k) at += s_cnt[k];
  for (long long i = lo; i < hi; ++i)
    if (e[i] > thr) idx[at++] = (int)i;
  if (t == 255) {
    int* m = meta + ((long long)b * R + r) * 3;
    m[0] = (int)nf;
    m[1] = at;
    m[2] = s_nz[0];
  }
}

// grid (frames, R (1 + NE), items), 256 threads.  y = r (1 + NE) + s: the mask of reference r over signal r (s = 0) or over
// estimate s - 1.  New frame m of the K kept ones: first half = the second half of kept frame m - 1 (if any) + the first
// half of kept frame m, second half = the second half of kept frame m + the first half of kept frame m + 1 (if any), each
// kept frame already under the window; the window again; zeros up to 512; radix-2 transform in LDS (thread t owns one
// butterfly per stage); band j = sqrt of the sum of |X|^2 over its bins, in bin order.
__global__ __launch_bounds__(256) void stoi_band_k(const double* x10, int NS, int R, long long n10, const double* table,
                                                   double* scratch, const int* meta) {
  __shared__ double re[ST_NFFT], im[ST_NFFT];
  const int NE = NS - R, r = blockIdx.y / (1 + NE), s = blockIdx.y % (1 + NE), b = blockIdx.z, t = threadIdx.x;
  const long long m = blockIdx.x;
  const int K = meta[((long long)b * R + r) * 3 + 1];
  if (m >= K) return;
  const StoiLay L = stoi_layout(NS, R, n10);
  const int* idx = reinterpret_cast<const int*>(scratch + (long long)b * L.total + L.idx) + (long long)r * L.nf;
  const double* x = x10 + ((long long)b * NS + (s == 0 ? r : R + s - 1)) * n10;
  const double* w = table + ST_T_WIN;
  const double* tw = table + ST_T_TW;
  {
    const long long i1 = idx[m];
    double v = w[t] * x[i1 * ST_HOP + t];
    if (t < ST_HOP) {
      if (m > 0) v = w[t + ST_HOP] * x[(long long)idx[m - 1] * ST_HOP + ST_HOP + t] + v;
    } else {
      if (m + 1 < K) v = v + w[t - ST_HOP] * x[(long long)idx[m + 1] * ST_HOP + t - ST_HOP];
    }
    const int at = (int)(__brev((unsigned)t) >> 23);                   // 9-bit reversal; t + 256 lands on at + 1
    re[at] = w[t] * v;
    re[at + 1] = 0.0;
    im[at] = 0.0;
    im[at + 1] = 0.0;
  }
#pragma unroll 1
  for (int st = 0; st < 9; ++st) {
    __syncthreads();
    const int half = 1 << st, k = t & (half - 1);
    const int i = ((t >> st) << (st + 1)) + k, j = i + half;
    const double c = tw[2 * (k << (8 - st))], sn = tw[2 * (k << (8 - st)) + 1];
    const double ur = re[i], ui = im[i], xr = re[j], xi = im[j];
    const double vr = xr * c + xi * sn, vi = xi * c - xr * sn;         // x (cos - i sin)
    re[i] = ur + vr;
    im[i] = ui + vi;
    re[j] = ur - vr;
    im[j] = ui - vi;
  }
  __syncthreads();
  if (t < ST_J) {
    double sum = 0.0;
    for (int k = ST_LO[t]; k < ST_HI[t]; ++k) sum += re[k] * re[k] + im[k] * im[k];
    scratch[(long long)b * L.total + L.tob + (((long long)r * (1 + NE) + s) * ST_J + t) * L.nf + m] = sqrt(sum);
  }
}

// grid (ceil(segments / 4), R NE, items), 256 threads: wave w takes segment 4 x + w of pair y = r NE + e.  Lanes 0 .. 14 own
// a band row each (30 frames in frame order), lanes 0 .. 29 a frame column each (15 bands in band order); lane 0 adds the 15
// row results and the 30 column results in index order.
__global__ __launch_bounds__(256) void stoi_seg_k(int NS, int R, long long n10, double* scratch, const int* meta) {
  __shared__ double sx[4][ST_J * ST_NSEG], sy[4][ST_J * ST_NSEG], red[4][ST_J + ST_NSEG];
  const int NE = NS - R, r = blockIdx.y / NE, e = blockIdx.y % NE, b = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const StoiLay L = stoi_layout(NS, R, n10);
  const int K = meta[((long long)b * R + r) * 3 + 1];
  const long long M = K - ST_NSEG + 1, m0 = (long long)blockIdx.x * 4 + wave;
  const bool active = m0 < M;
  double* X = sx[wave];
  double* Y = sy[wave];
  if (active) {
    const double* tx = scratch + (long long)b * L.total + L.tob + ((long long)r * (1 + NE)) * ST_J * L.nf + m0;
    const double* ty = tx + (long long)(1 + e) * ST_J * L.nf;
    for (int i = lane; i < ST_J * ST_NSEG; i += 64) {
      const int j = i / ST_NSEG, f = i % ST_NSEG;
      X[i] = tx[(long long)j * L.nf + f];
      Y[i] = ty[(long long)j * L.nf + f];
    }
  }
  __syncthreads();
  if (active && lane < ST_J) {
    double* xr = X + lane * ST_NSEG;
    double* yr = Y + lane * ST_NSEG;
    double sxx = 0.0, syy = 0.0, mx = 0.0, my = 0.0, mp = 0.0;
    for (int f = 0; f < ST_NSEG; ++f) {
      sxx += xr[f] * xr[f];
      syy += yr[f] * yr[f];
      mx += xr[f];
      my += yr[f];
    }
    const double c = sqrt(sxx) / (sqrt(syy) + ST_EPS);
    for (int f = 0; f < ST_NSEG; ++f) mp += fmin(c * yr[f], xr[f] * ST_CLIP);
    mx /= ST_NSEG;
    my /= ST_NSEG;
    mp /= ST_NSEG;
    double vx = 0.0, vy = 0.0, vp = 0.0;
    for (int f = 0; f < ST_NSEG; ++f) {
      const double a = xr[f] - mx, q = yr[f] - my, p = fmin(c * yr[f], xr[f] * ST_CLIP) - mp;
      vx += a * a;
      vy += q * q;
      vp += p * p;
    }
    const double dx = sqrt(vx) + ST_EPS, dy = sqrt(vy) + ST_EPS, dp = sqrt(vp) + ST_EPS;
    double d = 0.0;
    for (int f = 0; f < ST_NSEG; ++f) {
      const double a = (xr[f] - mx) / dx, p = (fmin(c * yr[f], xr[f] * ST_CLIP) - mp) / dp, q = (yr[f] - my) / dy;
      d += a * p;
      xr[f] = a;                                                       // the rows of ESTOI: minus the mean, over the norm
      yr[f] = q;
    }
    red[wave][lane] = d;
  }
  __syncthreads();
  if (active && lane < ST_NSEG) {
    double mx = 0.0, my = 0.0;
    for (int j = 0; j < ST_J; ++j) {
      mx += X[j * ST_NSEG + lane];
      my += Y[j * ST_NSEG + lane];
    }
    mx /= ST_J;
    my /= ST_J;
    double vx = 0.0, vy = 0.0;
    for (int j = 0; j < ST_J; ++j) {
      const double a = X[j * ST_NSEG + lane] - mx, q = Y[j * ST_NSEG + lane] - my;
      vx += a * a;
      vy += q * q;
    }
    const double dx = sqrt(vx) + ST_EPS, dy = sqrt(vy) + ST_EPS;
    double d = 0.0;
    for (int j = 0; j < ST_J; ++j) d += ((X[j * ST_NSEG + lane] - mx) / dx) * ((Y[j * ST_NSEG + lane] - my) / dy);
    red[wave][ST_J + lane] = d;
  }
  __syncthreads();
  if (active && lane == 0) {
    double ds = 0.0, de = 0.0;
    for (int j = 0; j < ST_J; ++j) ds += red[wave][j];
    for (int f = 0; f < ST_NSEG; ++f) de += red[wave][ST_J + f];
    double* q = scratch + (long long)b * L.total + L.part + (((long long)r * NE + e) * L.M + m0) * 2;
    q[0] = ds;
    q[1] = de;
  }
}

// grid (R NE, items), 256 threads.  Thread t adds segments t, t + 256, ... in that order; thread 0 adds the 256 partial sums
// in thread order.  out[item][estimate][reference] = (STOI, ESTOI); 1e-5 for both where fewer than 30 frames were kept.
__global__ __launch_bounds__(256) void stoi_fold_k(int NS, int R, long long n10, const double* scratch, const int* meta,
                                                   double* out) {
  __shared__ double s_s[256], s_e[256];
  const int NE = NS - R, r = blockIdx.x / NE, e = blockIdx.x % NE, b = blockIdx.y, t = threadIdx.x;
  const StoiLay L = stoi_layout(NS, R, n10);
  const long long M = (long long)meta[((long long)b * R + r) * 3 + 1] - ST_NSEG + 1;
  const double* q = scratch + (long long)b * L.total + L.part + ((long long)r * NE + e) * L.M * 2;
  double ds = 0.0, de = 0.0;
  for (long long m = t; m < M; m += 256) {
    ds += q[2 * m];
    de += q[2 * m + 1];
  }
  s_s[t] = ds;
  s_e[t] = de;
  __syncthreads();
  if (t == 0) {
    ds = 0.0;
    de = 0.0;
    for (int k = 0; k < 256; ++k) {
      ds += s_s[k];
      de += s_e[k];
    }
    double* o = out + (((long long)b * NE + e) * R + r) * 2;
    o[0] = M >= 1 ? ds / (double)(ST_J * M) : ST_SHORT;
    o[1] = M >= 1 ? de / (double)(ST_NSEG * M) : ST_SHORT;
  }
}

hipError_t launch_stoi_measure(const double* x10, const int* len10, int B, int NS, int R, long long n10, const double* table,
                               double* out, int* meta, double* scratch, hipStream_t s) {
  const StoiLay L = stoi_layout(NS, R, n10);
  const int NE = NS - R;
  const long long nf = stoi_frames(n10);
  hipError_t e;
  if (nf > 0) {
    hipLaunchKernelGGL(stoi_energy_k, dim3((unsigned)((nf + 3) / 4), R, B), dim3(256), 0, s, x10, len10, NS, R, n10, table,
                       scratch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(stoi_mask_k, dim3(R, B), dim3(256), 0, s, x10, len10, NS, R, n10, scratch, meta);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (nf >= ST_NSEG) {                                                 // fewer frames than one segment: nothing to transform
    hipLaunchKernelGGL(stoi_band_k, dim3((unsigned)nf, R * (1 + NE), B), dim3(256), 0, s, x10, NS, R, n10, table, scratch, meta);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(stoi_seg_k, dim3((unsigned)((L.M + 3) / 4), R * NE, B), dim3(256), 0, s, NS, R, n10, scratch, meta);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(stoi_fold_k, dim3(R * NE, B), dim3(256), 0, s, NS, R, n10, scratch, meta, out);
  return hipGetLastError();
}

}  // namespace mn
