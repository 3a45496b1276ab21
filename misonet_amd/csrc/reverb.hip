// Cepstral distance, log-likelihood ratio and frequency-weighted segmental SNR on the device: the figures the REVERB challenge
// judges dereverberation by (C ABI misonet_reverb_measure in api_score.hip; the definition is INTEGRATION.md 4j, restated in NumPy
// in tests/reverb_ref.py; the dataclass is formed in score.py).
//
//   rvb_level_k  P[item][signal] = sum of x^2 over the valid samples, every signal once (references, estimates, the mixture)
//   rvb_frame_k  one workgroup per (frame, signal, item): the frame through the strided views of misonet_score_wave, the window,
//                the transform in LDS, 25 cepstral coefficients, 23 mel band sums, 13 lags and Levinson-Durbin; 75 doubles per
//                frame (cepstrum, bands, lags, LPC, failed) to scratch, feature-major
//   rvb_pair_k   one workgroup per (estimate or mixture, reference, item): the used frames, the mean cepstral difference, the
//                three values of every frame, their means by a fixed tree and their medians by a radix selection on the
//                order-preserving bit pattern (integer LDS counters; exact for any number of frames)
//
// float64 throughout, no floating-point atomics, every sum in a fixed order, and an item never looks at another one: a result is
// bit-reproducible and does not depend on the batch it sits in or on its position there.
#include "kernels.hpp"

#include <cmath>

namespace mn {

constexpr int RV_NQ = 25, RV_NB = 23, RV_NL = 13;                    // cepstral coefficients, mel bands, lags (LPC order 12)
constexpr int RV_F_CEP = 0, RV_F_BAND = 25, RV_F_R = 48, RV_F_A = 61, RV_F_FAIL = 74, RV_NF = 75;
constexpr int RV_MAXFFT = 512, RV_MAXBIN = 257;
constexpr double RV_FLOOR = 1e-15, RV_CD_CAP = 10.0, RV_LLR_CAP = 2.0, RV_SNR_LO = -10.0, RV_SNR_HI = 35.0;
constexpr double RV_DB = 4.342944819032518;                         // 10 / ln 10
// the table: twiddles (cos, sin)(2 pi k / 512) [256][2], then per rate (16 kHz, 8 kHz) the window [N], the triangles
// [23][NFFT / 2 + 1] and the bins [lo, hi) outside which a triangle is zero, as doubles [23][2]
constexpr int RV_T_TW = 0, RV_T_RATE = 512;

struct RvbRate { int N, H, NFFT, LOG, nbin, off; };                  // off: where the rate's part of the table starts

__host__ __device__ inline int rvb_rate_doubles(int N, int nbin) { return N + RV_NB * nbin + 2 * RV_NB; }

static bool rvb_rate(int fs, RvbRate* r) {
  if (fs == 16000) { *r = {400, 160, 512, 9, 257, RV_T_RATE}; return true; }
  if (fs == 8000) { *r = {200, 80, 256, 8, 129, RV_T_RATE + rvb_rate_doubles(400, 257)}; return true; }
  return false;
}

int reverb_table_count() { return RV_T_RATE + rvb_rate_doubles(400, 257) + rvb_rate_doubles(200, 129); }

long long reverb_frames(long long n, int fs) {
  RvbRate r;
  if (!rvb_rate(fs, &r) || n < 1 || n > (1LL << 24)) return -1;
  return n >= r.N ? (n - r.N) / r.H + 1 : 0;
}

void reverb_build_table(double* t) {
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < RV_MAXFFT / 2; ++k) {
    t[RV_T_TW + 2 * k] = std::cos(2.0 * pi * k / RV_MAXFFT);
    t[RV_T_TW + 2 * k + 1] = std::sin(2.0 * pi * k / RV_MAXFFT);
  }
  const int rates[2] = {16000, 8000};
  for (int i = 0; i < 2; ++i) {
    RvbRate r;
    rvb_rate(rates[i], &r);
    double* w = t + r.off;
    double* tri = w + r.N;
    double* rng = tri + RV_NB * r.nbin;
    for (int k = 0; k < r.N; ++k) w[k] = 0.5 - 0.5 * std::cos(2.0 * pi * (k + 1) / (r.N + 1));
    // edges e_0 .. e_24 equally spaced in mel(f) = 2595 log10(1 + f / 700) from 0 to mel(fs / 2)
    double e[RV_NB + 2];
    const double top = 2595.0 * std::log10(1.0 + 0.5 * rates[i] / 700.0);
    for (int j = 0; j < RV_NB + 2; ++j) e[j] = 700.0 * (std::pow(10.0, (top * j / (RV_NB + 1)) / 2595.0) - 1.0);
    for (int b = 0; b < RV_NB; ++b) {
      int lo = r.nbin, hi = 0;
      for (int m = 0; m < r.nbin; ++m) {
        const double f = (double)m * rates[i] / r.NFFT;
        const double up = (f - e[b]) / (e[b + 1] - e[b]), down = (e[b + 2] - f) / (e[b + 2] - e[b + 1]);
        double h = up < down ? up : down;
        if (!(h > 0.0)) h = 0.0;
        tri[b * r.nbin + m] = h;
        if (h > 0.0) {
          if (m < lo) lo = m;
          hi = m + 1;
        }
      }
      if (hi <= lo) lo = hi = 0;
      rng[2 * b] = lo;
      rng[2 * b + 1] = hi;
    }
  }
}

// ---- the layout of an item's scratch, in doubles: P [NS], feat [NS][75][nf], val [NP][3][nf] ----------------------------------
struct RvbLay { long long nf, lvl, feat, val, total; };
__host__ __device__ inline RvbLay rvb_layout(int NS, int R, long long nfr) {
  RvbLay L;
  L.nf = nfr > 0 ? nfr : 1;
  L.lvl = 0;
  L.feat = L.lvl + NS;
  L.val = L.feat + (long long)NS * RV_NF * L.nf;
  L.total = L.val + (long long)(NS - R) * R * 3 * L.nf;
  return L;
}
long long reverb_item_doubles(int NS, int R, long long n, int fs) {
  const long long nfr = reverb_frames(n, fs);
  return nfr < 0 ? -1 : rvb_layout(NS, R, nfr).total;
}

// ---- the level -------------------------------------------------------------------------------------------------------------------
// grid (NS, items), 256 threads.  Signal s < R: reference s; s < R + E: estimate s - R; else the mixture.  Thread t adds the
// squares of samples t, t + 256, ... in that order, then the tree.
__global__ __launch_bounds__(256) void rvb_level_k(const SigView ref, const SigView est, const SigView mix, int R, int E, long long n,
                                                   const int* n_valid, long long nfr, double* scratch) {
  __shared__ double s_sum[256];
  const int s = blockIdx.x, b = blockIdx.y, NS = gridDim.x, t = threadIdx.x;
  const RvbLay L = rvb_layout(NS, R, nfr);
  const long long nv = sig_nv(n_valid, b, n);
  long long base;
  const SigView& v = sig_pick(ref, est, mix, R, E, s, b, &base);
  double acc = 0.0;
  for (long long m = t; m < nv; m += 256) {
    const double x = sig_load(v, base, m);
    acc += x * x;
  }
  const double P = sig_tree(s_sum, acc, t);
  if (t == 0) scratch[(long long)b * L.total + L.lvl + s] = P;
}

// ---- the features of a frame ---------------------------------------------------------------------------------------------------------
// grid (frames of n, NS, items), 256 threads.  The frame under the window, zeros up to NFFT, radix-2 transform in LDS (thread t
// owns one butterfly per stage; 128 threads at NFFT = 256), |X| and ln max(|X|, 1e-15) of bins 0 .. NFFT / 2.  Then wave w takes
// the cepstral coefficients q = w, w + 4, ... and the lags l = w, w + 4, ...: lane l adds its terms m = l, l + 64, ... in that
// order, 64-lane butterfly; threads 0 .. 22 add a band each in bin order; thread 0 runs Levinson-Durbin in LDS.
__global__ __launch_bounds__(256) void rvb_frame_k(const SigView ref, const SigView est, const SigView mix, int R, int E, long long n,
                                                   const int* n_valid, const RvbRate rt, long long nfr, const double* table,
                                                   double* scratch) {
  __shared__ double re[RV_MAXFFT], im[RV_MAXFFT], su[RV_MAXFFT], smag[RV_MAXBIN], slog[RV_MAXBIN];
  __shared__ double s_r[RV_NL], s_a[RV_NL], s_tmp[RV_NL], s_fail;
  const int s = blockIdx.y, b = blockIdx.z, NS = gridDim.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long fr = blockIdx.x;
  const long long nv = sig_nv(n_valid, b, n);
  const long long nfr_b = nv >= rt.N ? (nv - rt.N) / rt.H + 1 : 0;
  if (fr >= nfr_b) return;                                           // uniform over the workgroup
  const RvbLay L = rvb_layout(NS, R, nfr);
  long long base;
  const SigView& v = sig_pick(ref, est, mix, R, E, s, b, &base);
  const double* tw = table + RV_T_TW;
  const double* w = table + rt.off;
  const double* tri = w + rt.N;
  const double* rng = tri + RV_NB * rt.nbin;
  const int NFFT = rt.NFFT, N = rt.N, half_n = NFFT >> 1;
  for (int i = t; i < NFFT; i += 256) {
    const double u = i < N ? w[i] * sig_load(v, base, fr * rt.H + i) : 0.0;      // fr H + i <= nv - 1 by the frame count
    const int at = (int)(__brev((unsigned)i) >> (32 - rt.LOG));
    su[i] = u;
    re[at] = u;
    im[at] = 0.0;
  }
#pragma unroll 1
  for (int st = 0; st < rt.LOG; ++st) {
    __syncthreads();
    if (t < half_n) {
      const int half = 1 << st, k = t & (half - 1);
      const int i = ((t >> st) << (st + 1)) + k, j = i + half;
      const double c = tw[2 * (k << (8 - st))], sn = tw[2 * (k << (8 - st)) + 1];
      const double ur = re[i], ui = im[i], xr = re[j], xi = im[j];
      const double vr = xr * c + xi * sn, vi = xi * c - xr * sn;       // x (cos - i sin)
      re[i] = ur + vr;
      im[i] = ui + vi;
      re[j] = ur - vr;
      im[j] = ui - vi;
    }
  }
  __syncthreads();
  for (int m = t; m <= half_n; m += 256) {
    const double a = sqrt(re[m] * re[m] + im[m] * im[m]);
    smag[m] = a;
    slog[m] = log(a > RV_FLOOR ? a : RV_FLOOR);
  }
  __syncthreads();
  double* f = scratch + (long long)b * L.total + L.feat + (long long)s * RV_NF * L.nf + fr;
  // c[q] = (1 / NFFT) sum_{m < NFFT} l[m] cos(2 pi q m / NFFT), l extended evenly
  for (int q = wave; q < RV_NQ; q += 4) {
    double acc = 0.0;
    for (int m = lane; m < NFFT; m += 64) {
      const int k = ((q * m) & (NFFT - 1)) << (9 - rt.LOG);            // the angle in 512ths of a turn
      const double c = k < 256 ? tw[2 * k] : -tw[2 * (k - 256)];
      acc += slog[m <= half_n ? m : NFFT - m] * c;
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) acc += __shfl_xor(acc, k, 64);
    if (lane == 0) f[(long long)(RV_F_CEP + q) * L.nf] = acc / (double)NFFT;
  }
  // r[l] = sum_{k < N - l} u[k] u[k + l]
  for (int l = wave; l < RV_NL; l += 4) {
    double acc = 0.0;
    for (int k = lane; k < N - l; k += 64) acc += su[k] * su[k + l];
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) acc += __shfl_xor(acc, k, 64);
    if (lane == 0) {
      s_r[l] = acc;
      f[(long long)(RV_F_R + l) * L.nf] = acc;
    }
  }
  if (t < RV_NB) {
    const int lo = (int)rng[2 * t], hi = (int)rng[2 * t + 1];
    double acc = 0.0;
    for (int m = lo; m < hi; ++m) acc += tri[t * rt.nbin + m] * smag[m];
    f[(long long)(RV_F_BAND + t) * L.nf] = acc;
  }
  __syncthreads();
  if (t == 0) {
    // Levinson-Durbin: a[0] = 1, E_0 = r[0]; step k: lambda = -(sum_{j < k} a[j] r[k - j]) / E_{k-1}, a[j] += lambda a[k - j],
    // E_k = E_{k-1} (1 - lambda^2).  Failed: some E_0 .. E_12 is <= 0 or not finite.
    double err = s_r[0];
    bool fail = !(err > 0.0) || !isfinite(err);
    s_a[0] = 1.0;
    for (int k = 1; k < RV_NL; ++k) s_a[k] = 0.0;
    for (int k = 1; k < RV_NL && !fail; ++k) {
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc += s_a[j] * s_r[k - j];
      const double lam = -acc / err;
      for (int j = 0; j <= k; ++j) s_tmp[j] = s_a[j] + lam * s_a[k - j];
      for (int j = 0; j <= k; ++j) s_a[j] = s_tmp[j];
      err = err * (1.0 - lam * lam);
      fail = !(err > 0.0) || !isfinite(err);
    }
    s_fail = fail ? 1.0 : 0.0;
  }
  __syncthreads();
  if (t < RV_NL) f[(long long)(RV_F_A + t) * L.nf] = s_a[t];
  if (t == RV_NL) f[(long long)RV_F_FAIL * L.nf] = s_fail;
}

// ---- the pairs -----------------------------------------------------------------------------------------------------------------------
// the order-preserving bit pattern of a double that is not NaN, and back
__device__ __forceinline__ unsigned long long rvb_key(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double rvb_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFULL) : ~k));
}

// the k-th smallest (from 0) of the values of v[0 .. nf) that are not NaN; k must be below their number.  Eight passes over
// the bytes of the key from the top: a histogram of the values that share the prefix found so far, then the bin that holds
// rank k.  Every thread of the workgroup calls it and gets the value.
__device__ double rvb_select(const double* v, long long nf, int k, int* hist, int* pick, int t) {
  unsigned long long prefix = 0;
#pragma unroll 1
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    __syncthreads();
    hist[t] = 0;
    __syncthreads();
    for (long long i = t; i < nf; i += 256) {
      const double x = v[i];
      if (x == x) {
        const unsigned long long key = rvb_key(x);
        const bool in = pass == 0 ? true : (key >> (shift + 8)) == prefix;
        if (in) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
      }
    }
    __syncthreads();
    if (t == 0) {
      int c = 0, bin = 0;
      while (bin < 255 && c + hist[bin] <= k) c += hist[bin++];
      pick[0] = bin;
      pick[1] = k - c;
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned long long)pick[0];
    k = pick[1];
  }
  return rvb_unkey(prefix);
}

// v sorted ascending, K values: v[(K - 1) / 2] for odd K, (v[K / 2 - 1] + v[K / 2]) / 2 for even K
__device__ double rvb_median(const double* v, long long nf, int K, int* hist, int* pick, int t) {
  if (K & 1) return rvb_select(v, nf, (K - 1) / 2, hist, pick, t);
  const double lo = rvb_select(v, nf, K / 2 - 1, hist, pick, t), hi = rvb_select(v, nf, K / 2, hist, pick, t);
  return (lo + hi) / 2.0;
}

// Q(a, r) = sum_i sum_j a[i] a[j] r[|i - j|], rows in order
__device__ __forceinline__ double rvb_quad(const double (&a)[RV_NL], const double (&r)[RV_NL]) {
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < RV_NL; ++i) {
    double row = 0.0;
#pragma unroll
    for (int j = 0; j < RV_NL; ++j) row += a[j] * r[i > j ? i - j : j - i];
    q += a[i] * row;
  }
  return q;
}

// grid ((NS - R) R, items), 256 threads: pair y = e R + r, estimate (or, last, the mixture) e against reference r.  Thread t
// owns the frames t, t + 256, ... and adds them in that order; the threads are added by the tree.
// out[item][e][r] = (CD mean, CD median, LLR mean, LLR median, fwSegSNR mean, fwSegSNR median), count[item][e][r] = (frames, used
// frames, frames that count for LLR), val[item][e][r][3][nfr(n)] = the CD, LLR and fwSegSNR of every frame, NaN where not counted.
__global__ __launch_bounds__(256) void rvb_pair_k(int NS, int R, long long n, const int* n_valid, const RvbRate rt, long long nfr,
                                                  double* scratch, double* frame_out, double* out, int* count) {
  __shared__ double s_sum[256], s_dbar[RV_NQ];
  __shared__ int s_int[256], s_pick[2];
  const int NE = NS - R, e = blockIdx.x / R, r = blockIdx.x % R, b = blockIdx.y, t = threadIdx.x;
  const RvbLay L = rvb_layout(NS, R, nfr);
  const long long nv = sig_nv(n_valid, b, n);
  const long long nf = nv >= rt.N ? (nv - rt.N) / rt.H + 1 : 0;
  const double* item = scratch + (long long)b * L.total;
  const double* fx = item + L.feat + (long long)r * RV_NF * L.nf;
  const double* fy = item + L.feat + (long long)(R + e) * RV_NF * L.nf;
  const double Px = item[L.lvl + r], Py = item[L.lvl + R + e];
  const double gx = Px > 0.0 ? sqrt((double)nv / Px) : 0.0, gy = Py > 0.0 ? sqrt((double)nv / Py) : 0.0;
  const long long pair = ((long long)b * NE + e) * R + r;
  double* val = frame_out ? frame_out + pair * 3 * L.nf : scratch + (long long)b * L.total + L.val + (long long)blockIdx.x * 3 * L.nf;
  const double nan = __longlong_as_double(0x7FF8000000000000LL);

  int used = 0;
  for (long long i = t; i < nf; i += 256) used += fx[(long long)RV_F_R * L.nf + i] > 0.0;
  const int K = sig_tree(s_int, used, t);
  // the mean of d_t = c^x_t - c^y_t over the used frames
  for (int q = 0; q < RV_NQ; ++q) {
    double acc = 0.0;
    for (long long i = t; i < nf; i += 256)
      if (fx[(long long)RV_F_R * L.nf + i] > 0.0) acc += fx[(long long)(RV_F_CEP + q) * L.nf + i] - fy[(long long)(RV_F_CEP + q) * L.nf + i];
    const double sum = sig_tree(s_sum, acc, t);
    if (t == 0) s_dbar[q] = K > 0 ? sum / (double)K : 0.0;
  }
  __syncthreads();
  double a_cd = 0.0, a_llr = 0.0, a_fw = 0.0;
  int n_llr = 0;
  for (long long i = t; i < nf; i += 256) {
    double cd = nan, llr = nan, fw = nan;
    if (fx[(long long)RV_F_R * L.nf + i] > 0.0) {
      // CD
      double d2 = 0.0;
#pragma unroll 1
      for (int q = 1; q < RV_NQ; ++q) {
        const double d = fx[(long long)(RV_F_CEP + q) * L.nf + i] - fy[(long long)(RV_F_CEP + q) * L.nf + i] - s_dbar[q];
        d2 += d * d;
      }
      const double d0 = fx[(long long)RV_F_CEP * L.nf + i] - fy[(long long)RV_F_CEP * L.nf + i] - s_dbar[0];
      cd = RV_DB * sqrt(d0 * d0 + 2.0 * d2);
      cd = cd < RV_CD_CAP ? cd : RV_CD_CAP;
      a_cd += cd;
      // fwSegSNR
      double num = 0.0, den = 0.0;
#pragma unroll 1
      for (int k = 0; k < RV_NB; ++k) {
        const double xb = gx * fx[(long long)(RV_F_BAND + k) * L.nf + i], yb = gy * fy[(long long)(RV_F_BAND + k) * L.nf + i];
        const double wb = pow(xb, 0.2), df = xb - yb, dd = df * df;
        double snr = RV_SNR_HI;
        if (dd != 0.0) {
          snr = 10.0 * log10(xb * xb / dd);
          snr = snr > RV_SNR_LO ? snr : RV_SNR_LO;                     // log10(0) = -inf lands on the lower clip
          snr = snr < RV_SNR_HI ? snr : RV_SNR_HI;
        }
        num += wb * snr;
        den += wb;
      }
      fw = num / den;
      a_fw += fw;
      // LLR
      if (fx[(long long)RV_F_FAIL * L.nf + i] == 0.0 && fy[(long long)RV_F_FAIL * L.nf + i] == 0.0) {
        double ax[RV_NL], ay[RV_NL], rx[RV_NL];
#pragma unroll
        for (int k = 0; k < RV_NL; ++k) {
          ax[k] = fx[(long long)(RV_F_A + k) * L.nf + i];
          ay[k] = fy[(long long)(RV_F_A + k) * L.nf + i];
          rx[k] = fx[(long long)(RV_F_R + k) * L.nf + i];
        }
        const double qy = rvb_quad(ay, rx), qx = rvb_quad(ax, rx);
        if (qy > 0.0 && qx > 0.0) {
          llr = log(qy / qx);
          llr = llr > 0.0 ? llr : 0.0;
          llr = llr < RV_LLR_CAP ? llr : RV_LLR_CAP;
          a_llr += llr;
          n_llr += 1;
        }
      }
    }
    val[i] = cd;
    val[L.nf + i] = llr;
    val[2 * L.nf + i] = fw;
  }
  const double sum_cd = sig_tree(s_sum, a_cd, t), sum_llr = sig_tree(s_sum, a_llr, t), sum_fw = sig_tree(s_sum, a_fw, t);
  const int K_llr = sig_tree(s_int, n_llr, t);                     // its barriers also make val visible to the workgroup
  const bool valid = K >= 1 && Px > 0.0;
  double med_cd = nan, med_llr = nan, med_fw = nan;
  if (valid) {                                                         // uniform over the workgroup
    med_cd = rvb_median(val, nf, K, s_int, s_pick, t);
    med_fw = rvb_median(val + 2 * L.nf, nf, K, s_int, s_pick, t);
    if (K_llr > 0) med_llr = rvb_median(val + L.nf, nf, K_llr, s_int, s_pick, t);
  }
  if (t == 0) {
    double* o = out + pair * 6;
    o[0] = valid ? sum_cd / (double)K : nan;
    o[1] = med_cd;
    o[2] = valid && K_llr > 0 ? sum_llr / (double)K_llr : nan;
    o[3] = med_llr;
    o[4] = valid ? sum_fw / (double)K : nan;
    o[5] = med_fw;
    int* c = count + pair * 3;
    c[0] = (int)nf;
    c[1] = K;
    c[2] = K_llr;
  }
}

hipError_t launch_reverb_measure(const SigView& est, const SigView& ref, const SigView& mix, int B, int E, int R, long long n,
                                 const int* n_valid, int fs, const double* table, double* out, int* count, double* frame_out,
                                 double* scratch, hipStream_t s) {
  RvbRate rt;
  if (!rvb_rate(fs, &rt)) return hipErrorInvalidValue;
  const long long nfr = reverb_frames(n, fs);
  if (nfr < 0) return hipErrorInvalidValue;
  const int NS = R + E + (mix.p ? 1 : 0);
  hipError_t e;
  hipLaunchKernelGGL(rvb_level_k, dim3(NS, B), dim3(256), 0, s, ref, est, mix, R, E, n, n_valid, nfr, scratch);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (nfr > 0) {
    hipLaunchKernelGGL(rvb_frame_k, dim3((unsigned)nfr, NS, B), dim3(256), 0, s, ref, est, mix, R, E, n, n_valid, rt, nfr,
                       table, scratch);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(rvb_pair_k, dim3((NS - R) * R, B), dim3(256), 0, s, NS, R, n, n_valid, rt, nfr, scratch, frame_out, out, count);
  return hipGetLastError();
}

}  // namespace mn
