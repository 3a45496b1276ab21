// The speech-to-reverberation modulation energy ratio (SRMR, Falk, Zheng & Chan 2010) on the device: the one figure of the
// REVERB challenge that takes no clean reference (C ABI misonet_srmr_measure in api_score.hip; the definition is INTEGRATION.md
// 4k, restated in NumPy / SciPy in tests/srmr_ref.py; the dataclass is formed in score.py).
//
// A *pair* is one (item, signal, gammatone channel); the pairs of a call are numbered ((item NS + signal) 23 + channel) and run in
// groups of as many as 1 GiB of scratch holds.  Per group:
//
//   srmr_gt_k<1>      every chunk of C = 4096 samples of a pair through the 8th-order gammatone cascade from zero state; the 8
//                     final state values are kept
//   srmr_gt_sweep_k   one thread per pair walks its chunks: state <- A^C state + (zero-state final), A^C from the table; every
//                     chunk's true initial state replaces what pass 1 left
//   srmr_gt_k<2>      the chunks again from those states; the channel signal y goes to the pair's slot
//   srmr_hilbert_small_k / srmr_fft_col_k<fwd> + srmr_fft_row_k + srmr_fft_col_k<inv>
//                     env = |analytic signal| with P = the smallest power of two >= n: one LDS pass for P <= 4096, else the
//                     four-step split P = N1 N2 (N1 = 2^ceil(p/2)): N1-point transforms down the columns with the twiddles,
//                     then per row the N2-point transform, the one-sided mask, the inverse N2-point transform and the conjugate
//                     twiddles in one pass, then the inverse N1-point transforms down the columns with the magnitude.  Forward
//                     passes are decimation in frequency, inverse ones decimation in time, so no pass permutes anything: rows
//                     and bins simply sit in bit-reversed order in between.  env overwrites y.
//   srmr_mod_k<1>, srmr_mod_sweep_k, srmr_mod_k<2>
//                     the same chunked scan for the 8 second-order modulation filters; pass 2 never stores a filtered sample:
//                     per hop of H_w samples it keeps the four sums of (w[o + q H_w] v)^2, q = 0 .. 3 (N_w = 4 H_w, so frame t is
//                     hop t under the first window quarter, hop t + 1 under the second, ...)
//   srmr_energy_k     Ebar[j][k] = the mean over the frames of E_t, added hop by hop and by a fixed tree
//
// and once per call srmr_final_k: the 90 % bandwidth, K*, the ratio.  float64 throughout, the recurrences are evaluated as
// scipy.signal.lfilter evaluates them (transposed direct form II, no contraction to fused multiply-adds), no floating-point
// atomics, every sum in a fixed order, 64-bit sample indices, and a pair never looks at another one: a result is bit-reproducible
// and does not depend on the batch it sits in or on its position there.  P, the chunks and the frames of an item
// follow its own n_valid, and nothing beyond n_valid is read.
//
// LDS: a pass holds 4096 complex doubles as two planes (64 KB).  Column passes keep their columns interleaved (element (row, col)
// at row M + col), so a stage's butterflies read consecutive doubles whatever the stage; row passes run the early (inverse) and
// late (forward) stages at strides of 1, 2, 4 doubles, which costs bank conflicts on 3 of up to 12 stages.
#include "kernels.hpp"

#include <cmath>
#include <complex>

namespace mn {

constexpr int SR_NCH = 23, SR_NMOD = 8, SR_C = 4096, SR_LOGT = 12, SR_T = 1 << SR_LOGT;
constexpr long long SR_MAXN = 1LL << 24;
constexpr long long SR_SCRATCH_CAP = 1LL << 30;
// the table: W_4096^a (cos, sin) [4096][2], W_{2^24}^b [4096][2], then per rate (16 kHz, 8 kHz) the window [4096], the gammatone
// coefficients [23][8] = (gain, b0, a1, a2, b1 of the four sections), the gammatone transitions A^C [23][8][8], the modulation
// coefficients [8][4] = (b0, b2, a1, a2), their transitions [8][2][2], ERB(cf_j) [23], ll_k [8]
constexpr int SR_T_HI = 0, SR_T_LO = 2 * SR_T, SR_T_RATE = 4 * SR_T;
constexpr int SR_R_WIN = 0, SR_R_GTC = 4096, SR_R_GTA = SR_R_GTC + SR_NCH * 8, SR_R_MDC = SR_R_GTA + SR_NCH * 64,
              SR_R_MDA = SR_R_MDC + SR_NMOD * 4, SR_R_ERB = SR_R_MDA + SR_NMOD * 4, SR_R_LL = SR_R_ERB + SR_NCH,
              SR_R_TOTAL = SR_R_LL + SR_NMOD + 1;

static bool srmr_rate(int fs, int* Nw, int* Hw, int* off) {
  if (fs != 16000 && fs != 8000) return false;
  *Nw = (256 * fs + 999) / 1000;                                     // ceil(0.256 fs)
  *Hw = (64 * fs + 999) / 1000;
  *off = SR_T_RATE + (fs == 16000 ? 0 : SR_R_TOTAL);
  return true;
}

int srmr_table_count() { return SR_T_RATE + 2 * SR_R_TOTAL; }
int srmr_chunk() { return SR_C; }

long long srmr_frames(long long n, int fs) {
  int Nw, Hw, off;
  if (!srmr_rate(fs, &Nw, &Hw, &off) || n < 0 || n > SR_MAXN) return -1;
  return n >= Nw ? 1 + (n - Nw) / Hw : 0;
}

// one step of a biquad in transposed direct form II, in long double, for the transitions
static void sr_step_ld(long double* z, long double x, long double b0, long double b1, long double b2, long double a1,
                       long double a2, long double* y) {
  *y = z[0] + b0 * x;
  z[0] = z[1] + b1 * x - a1 * *y;
  z[1] = b2 * x - a2 * *y;
}

void srmr_build_table(double* t) {
  const double pi = 3.14159265358979323846;
  const long double pil = 3.14159265358979323846264338327950288L;
  for (int k = 0; k < SR_T; ++k) {
    t[SR_T_HI + 2 * k] = (double)cosl(2.0L * pil * k / 4096.0L);
    t[SR_T_HI + 2 * k + 1] = (double)sinl(2.0L * pil * k / 4096.0L);
    t[SR_T_LO + 2 * k] = (double)cosl(2.0L * pil * k / 16777216.0L);
    t[SR_T_LO + 2 * k + 1] = (double)sinl(2.0L * pil * k / 16777216.0L);
  }
  const int rates[2] = {16000, 8000};
  for (int ri = 0; ri < 2; ++ri) {
    const int fs = rates[ri];
    int Nw, Hw, off;
    srmr_rate(fs, &Nw, &Hw, &off);
    double* r = t + off;
    for (int i = 0; i < SR_R_TOTAL; ++i) r[i] = 0.0;
    for (int i = 0; i < Nw; ++i) r[SR_R_WIN + i] = 0.54 - 0.46 * std::cos(2.0 * pi * i / (Nw - 1));
    const double EarQ = 9.26449, minBW = 24.7, c = EarQ * minBW, T = 1.0 / fs;
    for (int j = 0; j < SR_NCH; ++j) {
      const int i = SR_NCH - j;                                       // ERBSpace descends; channel j ascends
      const double cf = -c + std::exp(i * (std::log(125.0 + c) - std::log(0.5 * fs + c)) / SR_NCH) * (0.5 * fs + c);
      const double erb = cf / EarQ + minBW, Bw = 1.019 * 2.0 * pi * erb;
      const double c1 = std::cos(2.0 * pi * cf * T), s1 = std::sin(2.0 * pi * cf * T), e = std::exp(-Bw * T);
      const double a1 = -2.0 * c1 * e, a2 = e * e, b0 = T;
      const double rr[4] = {std::sqrt(3.0 + std::pow(2.0, 1.5)), -std::sqrt(3.0 + std::pow(2.0, 1.5)),
                            std::sqrt(3.0 - std::pow(2.0, 1.5)), -std::sqrt(3.0 - std::pow(2.0, 1.5))};
      double* gc = r + SR_R_GTC + j * 8;
      std::complex<double> H(1.0, 0.0);
      const std::complex<double> zi = std::exp(std::complex<double>(0.0, -2.0 * pi * cf * T));     // z^-1 at cf
      for (int s = 0; s < 4; ++s) {
        gc[4 + s] = -(2.0 * T * c1 * e + 2.0 * rr[s] * T * s1 * e) / 2.0;
        H *= (b0 + gc[4 + s] * zi) / (1.0 + a1 * zi + a2 * zi * zi);
      }
      gc[0] = 1.0 / std::abs(H);
      gc[1] = b0;
      gc[2] = a1;
      gc[3] = a2;
      r[SR_R_ERB + j] = erb;
      // column q of A^C: the state after C steps of zero input from the unit state q
      for (int q = 0; q < 8; ++q) {
        long double z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        z[q] = 1.0L;
        for (int m = 0; m < SR_C; ++m) {
          long double x = 0.0L, y;
          for (int s = 0; s < 4; ++s) {
            sr_step_ld(z + 2 * s, x, b0, gc[4 + s], 0.0L, a1, a2, &y);
            x = y;
          }
        }
        for (int p = 0; p < 8; ++p) r[SR_R_GTA + j * 64 + p * 8 + q] = (double)z[p];
      }
    }
    for (int k = 0; k < SR_NMOD; ++k) {
      const double fk = 4.0 * std::pow(32.0, k / 7.0), W = std::tan(pi * fk / fs), beta = W / 2.0;
      const double a0 = 1.0 + beta + W * W;
      double* mc = r + SR_R_MDC + k * 4;
      mc[0] = beta / a0;
      mc[1] = -beta / a0;
      mc[2] = (2.0 * W * W - 2.0) / a0;
      mc[3] = (1.0 - beta + W * W) / a0;
      r[SR_R_LL + k] = fk - beta * fs / (2.0 * pi);
      for (int q = 0; q < 2; ++q) {
        long double z[2] = {0, 0}, y;
        z[q] = 1.0L;
        for (int m = 0; m < SR_C; ++m) sr_step_ld(z, 0.0L, mc[0], 0.0L, mc[1], mc[2], mc[3], &y);
        for (int p = 0; p < 2; ++p) r[SR_R_MDA + k * 4 + p * 2 + q] = (double)z[p];
      }
    }
  }
}

// ---- the layout of a pair's slot, in doubles: y / env [n], Z complex [P] (four-step route only), the gammatone states
// [chunks][8], the modulation states [chunks][8][2], the hop sums [hops][4][8] ------------------------------------------------
struct SrmrLay { long long nch, nh, o_z, o_gst, o_mst, o_hp, slot; };
static SrmrLay srmr_layout(long long n, int Hw) {
  SrmrLay L;
  long long P = 1;
  while (P < n) P <<= 1;
  L.nch = (n + SR_C - 1) / SR_C;
  L.nh = (n + Hw - 1) / Hw;
  L.o_z = (n + 1) / 2 * 2;
  L.o_gst = L.o_z + (P > SR_T ? 2 * P : 0);
  L.o_mst = L.o_gst + L.nch * 8;
  L.o_hp = L.o_mst + L.nch * SR_NMOD * 2;
  L.slot = L.o_hp + L.nh * 4 * SR_NMOD;
  return L;
}
static long long srmr_group(long long pairs, long long slot) {
  long long fit = SR_SCRATCH_CAP / (8 * slot);
  if (fit > 32768) fit = 32768;                                        // a group is also one grid dimension
  return fit < 1 ? 1 : (fit < pairs ? fit : pairs);
}
long long srmr_scratch_doubles(int B, int NS, long long n, int fs) {
  int Nw, Hw, off;
  if (!srmr_rate(fs, &Nw, &Hw, &off) || B < 1 || B > 4096 || NS < 1 || NS > 5 || n < 1 || n > SR_MAXN) return -1;
  const SrmrLay L = srmr_layout(n, Hw);
  const long long pairs = (long long)B * NS * SR_NCH;
  return pairs * SR_NMOD + srmr_group(pairs, L.slot) * L.slot;
}

struct SrmrArgs {
  SigView sig, mix;
  int S, NS, Nw, Hw;
  long long n;
  const int* n_valid;
  const double* tab;                                                   // the whole table
  const double* rt;                                                    // the rate's part
  SrmrLay L;
  double* ebar;                                                        // [B][NS][23][8]
  double* slots;
};

__device__ __forceinline__ long long sr_nv(const SrmrArgs& a, int b) { return sig_nv(a.n_valid, b, a.n); }
__device__ __forceinline__ int sr_log2_ceil(long long nv) {              // p with 2^p the smallest power of two >= nv (nv >= 1)
  return nv <= 1 ? 0 : 64 - __clzll((unsigned long long)(nv - 1));
}
struct SrmrPair { int b, s, j; };
__device__ __forceinline__ SrmrPair sr_pair(const SrmrArgs& a, long long g) {
  SrmrPair p;
  p.j = (int)(g % SR_NCH);
  const long long bs = g / SR_NCH;
  p.s = (int)(bs % a.NS);
  p.b = (int)(bs / a.NS);
  return p;
}

// ---- the gammatone cascade --------------------------------------------------------------------------------------------------------
// one thread per (pair of the group, chunk), pairs fastest: the lanes of a wave are the channels of one signal at one chunk and
// read the same samples.  PASS 1 leaves the final state of a zero-state run (not of an item's last chunk: nothing follows it),
// PASS 2 starts from the state the sweep left and writes y.
template <int PASS>
__global__ __launch_bounds__(64) void srmr_gt_k(const SrmrArgs a, long long g0, int np) {
#pragma clang fp contract(off)
  const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
  if (id >= (long long)np * a.L.nch) return;
  const int pi = (int)(id % np);
  const long long c = id / np;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  const long long m0 = c * SR_C;
  if (nv < a.Nw || m0 >= nv) return;
  if (PASS == 1 && m0 + SR_C >= nv) return;
  const int len = (int)(nv - m0 < SR_C ? nv - m0 : SR_C);
  const double* gc = a.rt + SR_R_GTC + pr.j * 8;
  const double gain = gc[0], b0 = gc[1], a1 = gc[2], a2 = gc[3];
  const double b10 = gc[4], b11 = gc[5], b12 = gc[6], b13 = gc[7];
  double* slot = a.slots + (long long)pi * a.L.slot;
  double* st = slot + a.L.o_gst + c * 8;
  double z00 = 0, z01 = 0, z10 = 0, z11 = 0, z20 = 0, z21 = 0, z30 = 0, z31 = 0;
  if (PASS == 2) {
    z00 = st[0]; z01 = st[1]; z10 = st[2]; z11 = st[3]; z20 = st[4]; z21 = st[5]; z30 = st[6]; z31 = st[7];
  }
  long long base;
  const SigView& v = sig_pick(a.sig, a.sig, a.mix, 0, a.S, pr.s, pr.b, &base);
  double* y = slot + m0;
#pragma unroll 1
  for (int i = 0; i < len; ++i) {
    const double x = sig_load(v, base, m0 + i) * gain;
    const double y0 = z00 + b0 * x;
    z00 = z01 + b10 * x - a1 * y0;
    z01 = -(a2 * y0);
    const double y1 = z10 + b0 * y0;
    z10 = z11 + b11 * y0 - a1 * y1;
    z11 = -(a2 * y1);
    const double y2 = z20 + b0 * y1;
    z20 = z21 + b12 * y1 - a1 * y2;
    z21 = -(a2 * y2);
    const double y3 = z30 + b0 * y2;
    z30 = z31 + b13 * y2 - a1 * y3;
    z31 = -(a2 * y3);
    if (PASS == 2) y[i] = y3;
  }
  if (PASS == 1) {
    st[0] = z00; st[1] = z01; st[2] = z10; st[3] = z11; st[4] = z20; st[5] = z21; st[6] = z30; st[7] = z31;
  }
}

// one thread per pair of the group: chunk c's entry becomes the state the chunk starts from
__global__ __launch_bounds__(64) void srmr_gt_sweep_k(const SrmrArgs a, long long g0, int np) {
  const int pi = blockIdx.x * 64 + threadIdx.x;
  if (pi >= np) return;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  if (nv < a.Nw) return;
  const long long nch = (nv + SR_C - 1) / SR_C;
  const double* A = a.rt + SR_R_GTA + pr.j * 64;
  double* st = a.slots + (long long)pi * a.L.slot + a.L.o_gst;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
#pragma unroll 1
  for (long long c = 0; c < nch; ++c) {
    double* e = st + c * 8;
    double f[8], nx[8];
    const bool more = c + 1 < nch;
#pragma unroll
    for (int r = 0; r < 8; ++r) f[r] = more ? e[r] : 0.0;
    e[0] = s0; e[1] = s1; e[2] = s2; e[3] = s3; e[4] = s4; e[5] = s5; e[6] = s6; e[7] = s7;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const double* ar = A + r * 8;
      double acc = ar[0] * s0;
      acc += ar[1] * s1; acc += ar[2] * s2; acc += ar[3] * s3; acc += ar[4] * s4; acc += ar[5] * s5; acc += ar[6] * s6;
      acc += ar[7] * s7;
      nx[r] = acc + f[r];
    }
    s0 = nx[0]; s1 = nx[1]; s2 = nx[2]; s3 = nx[3]; s4 = nx[4]; s5 = nx[5]; s6 = nx[6]; s7 = nx[7];
  }
}

// ---- the transform passes in LDS -----------------------------------------------------------------------------------------------------
// T <= 4096 complex doubles in re[] / im[] hold 2^logM interleaved sequences of N = 2^logN points each (logM = 0: sequences of N
// consecutive points, T / N of them).  Forward: decimation in frequency, natural order in, bit-reversed out, W = exp(-2 pi i / N);
// inverse: decimation in time, bit-reversed in, natural out, the conjugate twiddles, no scaling.  256 threads; ends on a barrier.
template <bool INV>
__device__ __forceinline__ void sr_fft(double* re, double* im, int T, int logN, int logM, const double* thi, int t) {
#pragma unroll 1
  for (int q = 0; q < logN; ++q) {
    const int s = INV ? q : logN - 1 - q;
    const int sh = s + logM;
    __syncthreads();
    for (int u = t; u < (T >> 1); u += 256) {
      const int kk = u & ((1 << sh) - 1);
      const int i = ((u >> sh) << (sh + 1)) + kk, j = i + (1 << sh);
      const int tw = (kk >> logM) << (11 - s);
      const double c = thi[2 * tw], sn = thi[2 * tw + 1];
      const double ar = re[i], ai = im[i], br = re[j], bi = im[j];
      if (INV) {
        const double vr = br * c - bi * sn, vi = bi * c + br * sn;
        re[i] = ar + vr; im[i] = ai + vi;
        re[j] = ar - vr; im[j] = ai - vi;
      } else {
        const double dr = ar - br, di = ai - bi;
        re[i] = ar + br; im[i] = ai + bi;
        re[j] = dr * c + di * sn; im[j] = di * c - dr * sn;
      }
    }
  }
  __syncthreads();
}
// the weight of bin k of P in the analytic signal, with the 1 / P of the inverse transform
__device__ __forceinline__ double sr_mask(long long k, int p) {
  const long long half = 1LL << (p - 1);
  const double f = (k == 0 || k == half) ? 1.0 : (k < half ? 2.0 : 0.0);
  return f / (double)(1LL << p);
}
// W_P^m = exp(-2 pi i m / P), P = 2^p <= 2^24, 0 <= m < P, from the two tables
__device__ __forceinline__ void sr_twiddle(const double* tab, long long m, int p, double* c, double* s) {
  const long long ex = m << (24 - p);
  const int hi = (int)(ex >> 12), lo = (int)(ex & 4095);
  const double ch = tab[SR_T_HI + 2 * hi], sh = tab[SR_T_HI + 2 * hi + 1];
  const double cl = tab[SR_T_LO + 2 * lo], sl = tab[SR_T_LO + 2 * lo + 1];
  *c = ch * cl - sh * sl;
  *s = sh * cl + ch * sl;
}
__device__ __forceinline__ unsigned sr_brev(unsigned x, int bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// grid (1, pairs of the group): P <= 4096 in one pass
__global__ __launch_bounds__(256) void srmr_hilbert_small_k(const SrmrArgs a, long long g0) {
  __shared__ double re[SR_T], im[SR_T];
  const int pi = blockIdx.y, t = threadIdx.x;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  const int p = sr_log2_ceil(nv);
  if (nv < a.Nw || p > SR_LOGT) return;
  const int P = 1 << p;
  double* y = a.slots + (long long)pi * a.L.slot;
  for (int e = t; e < P; e += 256) {
    re[e] = e < nv ? y[e] : 0.0;
    im[e] = 0.0;
  }
  sr_fft<false>(re, im, P, p, 0, a.tab + SR_T_HI, t);
  for (int e = t; e < P; e += 256) {
    const double f = sr_mask(sr_brev((unsigned)e, p), p);
    re[e] *= f;
    im[e] *= f;
  }
  sr_fft<true>(re, im, P, p, 0, a.tab + SR_T_HI, t);
  for (int e = t; e < P; e += 256)
    if (e < nv) y[e] = sqrt(re[e] * re[e] + im[e] * im[e]);
}

// grid (P of n / 4096, pairs of the group): tile x holds the M = 4096 / N1 columns x M .. x M + M - 1 of the N1 x N2 array.
// Forward: y (zeros from n_valid on) -> N1-point transform down each column -> times W_P^(n2 k1) -> Z[r][n2], row r holding
// k1 = bitrev(r).  Inverse: Z -> inverse N1-point transform -> env = the magnitude, over y.
template <bool INV>
__global__ __launch_bounds__(256) void srmr_fft_col_k(const SrmrArgs a, long long g0) {
  __shared__ double re[SR_T], im[SR_T];
  const int pi = blockIdx.y, t = threadIdx.x;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  const int p = sr_log2_ceil(nv);
  if (nv < a.Nw || p <= SR_LOGT || (long long)blockIdx.x >= (1LL << (p - SR_LOGT))) return;
  const int p1 = (p + 1) >> 1, p2 = p - p1, logM = SR_LOGT - p1, M = 1 << logM;
  const long long col0 = (long long)blockIdx.x << logM;
  double* y = a.slots + (long long)pi * a.L.slot;
  double2* Z = reinterpret_cast<double2*>(y + a.L.o_z);
  for (int e = t; e < SR_T; e += 256) {
    const long long row = e >> logM, at = (row << p2) + col0 + (e & (M - 1));
    if (INV) {
      const double2 z = Z[at];
      re[e] = z.x;
      im[e] = z.y;
    } else {
      re[e] = at < nv ? y[at] : 0.0;
      im[e] = 0.0;
    }
  }
  sr_fft<INV>(re, im, SR_T, p1, logM, a.tab + SR_T_HI, t);
  for (int e = t; e < SR_T; e += 256) {
    const long long row = e >> logM, n2 = col0 + (e & (M - 1)), at = (row << p2) + n2;
    if (INV) {
      if (at < nv) y[at] = sqrt(re[e] * re[e] + im[e] * im[e]);
    } else {
      double c, s;
      sr_twiddle(a.tab, n2 * (long long)sr_brev((unsigned)row, p1), p, &c, &s);
      Z[at] = make_double2(re[e] * c + im[e] * s, im[e] * c - re[e] * s);
    }
  }
}

// grid (P of n / 4096, pairs of the group): 4096 consecutive elements of Z = 4096 / N2 whole rows.  Per row r (k1 = bitrev(r)):
// the N2-point transform, the mask of bin k1 + N1 bitrev(position) with 1 / P, the inverse transform, times conj W_P^(n2 k1).
__global__ __launch_bounds__(256) void srmr_fft_row_k(const SrmrArgs a, long long g0) {
  __shared__ double re[SR_T], im[SR_T];
  const int pi = blockIdx.y, t = threadIdx.x;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  const int p = sr_log2_ceil(nv);
  if (nv < a.Nw || p <= SR_LOGT || (long long)blockIdx.x >= (1LL << (p - SR_LOGT))) return;
  const int p1 = (p + 1) >> 1, p2 = p - p1;
  const long long base = (long long)blockIdx.x << SR_LOGT;
  double2* Z = reinterpret_cast<double2*>(a.slots + (long long)pi * a.L.slot + a.L.o_z) + base;
  for (int e = t; e < SR_T; e += 256) {
    const double2 z = Z[e];
    re[e] = z.x;
    im[e] = z.y;
  }
  sr_fft<false>(re, im, SR_T, p2, 0, a.tab + SR_T_HI, t);
  for (int e = t; e < SR_T; e += 256) {
    const long long k1 = sr_brev((unsigned)((base + e) >> p2), p1), k2 = sr_brev((unsigned)(e & ((1 << p2) - 1)), p2);
    const double f = sr_mask(k1 + (k2 << p1), p);
    re[e] *= f;
    im[e] *= f;
  }
  sr_fft<true>(re, im, SR_T, p2, 0, a.tab + SR_T_HI, t);
  for (int e = t; e < SR_T; e += 256) {
    const long long k1 = sr_brev((unsigned)((base + e) >> p2), p1), n2 = e & ((1 << p2) - 1);
    double c, s;
    sr_twiddle(a.tab, n2 * k1, p, &c, &s);
    Z[e] = make_double2(re[e] * c - im[e] * s, im[e] * c + re[e] * s);
  }
}

// ---- the modulation filters and the hop sums -----------------------------------------------------------------------------------------
// one thread per (filter, pair of the group, chunk), filters fastest: eight lanes read the same envelope sample
template <int PASS>
__global__ __launch_bounds__(64) void srmr_mod_k(const SrmrArgs a, long long g0, int np) {
#pragma clang fp contract(off)
  const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
  if (id >= (long long)np * SR_NMOD * a.L.nch) return;
  const int k = (int)(id % SR_NMOD), pi = (int)((id / SR_NMOD) % np);
  const long long c = id / ((long long)SR_NMOD * np);
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  const long long m0 = c * SR_C;
  if (nv < a.Nw || m0 >= nv) return;
  if (PASS == 1 && m0 + SR_C >= nv) return;
  const double* mc = a.rt + SR_R_MDC + k * 4;
  const double b0 = mc[0], b2 = mc[1], a1 = mc[2], a2 = mc[3];
  double* slot = a.slots + (long long)pi * a.L.slot;
  double* st = slot + a.L.o_mst + (c * SR_NMOD + k) * 2;
  const double* env = slot;
  double z0 = 0.0, z1 = 0.0;
  if (PASS == 1) {
    const int len = (int)(nv - m0 < SR_C ? nv - m0 : SR_C);
#pragma unroll 1
    for (int i = 0; i < len; ++i) {
      const double x = env[m0 + i];
      const double y = z0 + b0 * x;
      z0 = z1 - a1 * y;
      z1 = b2 * x - a2 * y;
    }
    st[0] = z0;
    st[1] = z1;
  } else {
    z0 = st[0];
    z1 = st[1];
    const int H = a.Hw;
    const double* w = a.rt + SR_R_WIN;
    double* hp = slot + a.L.o_hp;
#pragma unroll 1
    for (long long h = m0 / H; h < (m0 + SR_C) / H; ++h) {
      const long long mh = h * H;
      if (mh + H > nv) break;                                          // an incomplete hop belongs to no frame
      double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
#pragma unroll 1
      for (int o = 0; o < H; ++o) {
        const double x = env[mh + o];
        const double y = z0 + b0 * x;
        z0 = z1 - a1 * y;
        z1 = b2 * x - a2 * y;
        const double v0 = w[o] * y, v1 = w[o + H] * y, v2 = w[o + 2 * H] * y, v3 = w[o + 3 * H] * y;
        e0 += v0 * v0;
        e1 += v1 * v1;
        e2 += v2 * v2;
        e3 += v3 * v3;
      }
      double* out = hp + (h * 4) * SR_NMOD + k;
      out[0] = e0;
      out[SR_NMOD] = e1;
      out[2 * SR_NMOD] = e2;
      out[3 * SR_NMOD] = e3;
    }
  }
}

__global__ __launch_bounds__(64) void srmr_mod_sweep_k(const SrmrArgs a, long long g0, int np) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= np * SR_NMOD) return;
  const int k = id % SR_NMOD, pi = id / SR_NMOD;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  if (nv < a.Nw) return;
  const long long nch = (nv + SR_C - 1) / SR_C;
  const double* A = a.rt + SR_R_MDA + k * 4;
  const double a00 = A[0], a01 = A[1], a10 = A[2], a11 = A[3];
  double* st = a.slots + (long long)pi * a.L.slot + a.L.o_mst + k * 2;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 1
  for (long long c = 0; c < nch; ++c) {
    double* e = st + c * SR_NMOD * 2;
    const bool more = c + 1 < nch;
    const double f0 = more ? e[0] : 0.0, f1 = more ? e[1] : 0.0;
    e[0] = s0;
    e[1] = s1;
    const double n0 = a00 * s0 + a01 * s1 + f0, n1 = a10 * s0 + a11 * s1 + f1;
    s0 = n0;
    s1 = n1;
  }
}

// grid (pairs of the group), 256 threads.  Ebar[j][k] = (1 / frames) sum over the hops h of (sum over q = 0 .. 3 with
// 0 <= h - q < frames of the hop sum (h, q)): thread t adds hops t, t + 256, ... in that order, then a fixed tree.
__global__ __launch_bounds__(256) void srmr_energy_k(const SrmrArgs a, long long g0) {
  __shared__ double s_sum[256];
  const int pi = blockIdx.x, t = threadIdx.x;
  const SrmrPair pr = sr_pair(a, g0 + pi);
  const long long nv = sr_nv(a, pr.b);
  if (nv < a.Nw) return;
  const long long nfr = 1 + (nv - a.Nw) / a.Hw;
  const double* hp = a.slots + (long long)pi * a.L.slot + a.L.o_hp;
#pragma unroll 1
  for (int k = 0; k < SR_NMOD; ++k) {
    double acc = 0.0;
    for (long long h = t; h < nfr + 3; h += 256) {
      double e = 0.0;
      for (int q = 0; q < 4; ++q)
        if (h - q >= 0 && h - q < nfr) e += hp[(h * 4 + q) * SR_NMOD + k];
      acc += e;
    }
    __syncthreads();
    s_sum[t] = acc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
      if (t < d) s_sum[t] += s_sum[t + d];
      __syncthreads();
    }
    if (t == 0) a.ebar[(g0 + pi) * SR_NMOD + k] = s_sum[0] / (double)nfr;
  }
}

// grid (B NS), 64 threads of which one works: the 184 means of a signal -> (SRMR, K*, BW), the frames, the means themselves
__global__ __launch_bounds__(64) void srmr_final_k(const SrmrArgs a, double* out, int* count, double* energy) {
  __shared__ double s_a[SR_NCH];
  if (threadIdx.x) return;
  const long long bs = blockIdx.x;
  const long long nv = sr_nv(a, (int)(bs / a.NS));
  const long long nfr = nv >= a.Nw ? 1 + (nv - a.Nw) / a.Hw : 0;
  const double* E = a.ebar + bs * SR_NCH * SR_NMOD;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  count[bs] = (int)nfr;
  double tot = 0.0;
  if (nfr >= 1) {
    for (int j = 0; j < SR_NCH; ++j) {
      double s = 0.0;
      for (int k = 0; k < SR_NMOD; ++k) s += E[j * SR_NMOD + k];
      s_a[j] = s;
      tot += s;
    }
  }
  const bool valid = nfr >= 1 && tot > 0.0;
  if (energy)
    for (int i = 0; i < SR_NCH * SR_NMOD; ++i) energy[bs * SR_NCH * SR_NMOD + i] = nfr >= 1 ? E[i] : nan;
  if (!valid) {
    out[bs * 3] = nan;
    out[bs * 3 + 1] = 0.0;
    out[bs * 3 + 2] = nan;
    return;
  }
  int jstar = 0;
  double run = 0.0;
  for (int j = SR_NCH - 1; j >= 0; --j) {
    run += 100.0 * s_a[j] / tot;
    if (run > 90.0) {
      jstar = j;
      break;
    }
  }
  const double bw = a.rt[SR_R_ERB + jstar];
  const double* ll = a.rt + SR_R_LL;
  const int K = 5 + (bw >= ll[5] ? 1 : 0) + (bw >= ll[6] ? 1 : 0) + (bw >= ll[7] ? 1 : 0);
  double num = 0.0, den = 0.0;
  for (int j = 0; j < SR_NCH; ++j) {
    for (int k = 0; k < 4; ++k) num += E[j * SR_NMOD + k];
    for (int k = 4; k < K; ++k) den += E[j * SR_NMOD + k];
  }
  out[bs * 3] = num / den;
  out[bs * 3 + 1] = (double)K;
  out[bs * 3 + 2] = bw;
}

hipError_t launch_srmr_measure(const SigView& sig, const SigView& mix, int B, int S, long long n, const int* n_valid, int fs,
                               const double* table, double* out, int* count, double* energy, double* scratch, hipStream_t s) {
  SrmrArgs a;
  int off;
  if (!srmr_rate(fs, &a.Nw, &a.Hw, &off)) return hipErrorInvalidValue;
  a.sig = sig;
  a.mix = mix;
  a.S = S;
  a.NS = S + (mix.p ? 1 : 0);
  a.n = n;
  a.n_valid = n_valid;
  a.tab = table;
  a.rt = table + off;
  a.L = srmr_layout(n, a.Hw);
  const long long pairs = (long long)B * a.NS * SR_NCH;
  const long long G = srmr_group(pairs, a.L.slot);
  a.ebar = scratch;
  a.slots = scratch + pairs * SR_NMOD;
  if (n >= a.Nw) {
    long long P = 1;
    while (P < n) P <<= 1;
    const unsigned tiles = (unsigned)(P >> SR_LOGT);
    for (long long g0 = 0; g0 < pairs; g0 += G) {
      const int np = (int)(pairs - g0 < G ? pairs - g0 : G);
      const unsigned gt_blocks = (unsigned)(((long long)np * a.L.nch + 63) / 64);
      const unsigned md_blocks = (unsigned)(((long long)np * SR_NMOD * a.L.nch + 63) / 64);
      if (a.L.nch > 1) hipLaunchKernelGGL(srmr_gt_k<1>, dim3(gt_blocks), dim3(64), 0, s, a, g0, np);
      hipLaunchKernelGGL(srmr_gt_sweep_k, dim3((np + 63) / 64), dim3(64), 0, s, a, g0, np);
      hipLaunchKernelGGL(srmr_gt_k<2>, dim3(gt_blocks), dim3(64), 0, s, a, g0, np);
      if (tiles >= 2) {
        hipLaunchKernelGGL(srmr_fft_col_k<false>, dim3(tiles, np), dim3(256), 0, s, a, g0);
        hipLaunchKernelGGL(srmr_fft_row_k, dim3(tiles, np), dim3(256), 0, s, a, g0);
        hipLaunchKernelGGL(srmr_fft_col_k<true>, dim3(tiles, np), dim3(256), 0, s, a, g0);
      }
      if (tiles < 2 || n_valid) hipLaunchKernelGGL(srmr_hilbert_small_k, dim3(1, np), dim3(256), 0, s, a, g0);
      if (a.L.nch > 1) hipLaunchKernelGGL(srmr_mod_k<1>, dim3(md_blocks), dim3(64), 0, s, a, g0, np);
      hipLaunchKernelGGL(srmr_mod_sweep_k, dim3((np * SR_NMOD + 63) / 64), dim3(64), 0, s, a, g0, np);
      hipLaunchKernelGGL(srmr_mod_k<2>, dim3(md_blocks), dim3(64), 0, s, a, g0, np);
      hipLaunchKernelGGL(srmr_energy_k, dim3(np), dim3(256), 0, s, a, g0);
    }
  }
  hipLaunchKernelGGL(srmr_final_k, dim3((unsigned)(B * a.NS)), dim3(64), 0, s, a, out, count, energy);
  return hipGetLastError();
}

}  // namespace mn
