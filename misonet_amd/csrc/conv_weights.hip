// Weight images of the 3x3 conv kernels: one packer per ConvKind (conv_select.hpp), from a layer's Conv2d / ConvTranspose2d weights
// to the layout its kernel reads.  Host code only; misonet_net_commit (net.hip) places the images in the device weight arena.
#include "conv_select.hpp"

#include <math.h>
#include <cmath>
#include <algorithm>
#include <string.h>

namespace mn {

// tap (kt, kf) of (co, ci) in conv form: a ConvTranspose2d weight is [Cin][Cout][3][3] with the taps flipped
static inline float tap(const ConvWeights& c, int co, int ci, int kt, int kf) {
  return c.transposed ? c.W[(((long long)ci * c.Cout + co) * 3 + (2 - kt)) * 3 + (2 - kf)]
                      : c.W[(((long long)co * c.Cin + ci) * 3 + kt) * 3 + kf];
}
static const double WINO_G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
// U = G g G^T of (co, ci) at position (xi along frequency, nu along time), in double
static inline double wino_u(const ConvWeights& c, int co, int ci, int xi, int nu) {
  double u = 0.0;
  for (int kt = 0; kt < 3; ++kt)
    for (int kf = 0; kf < 3; ++kf) u += WINO_G[xi][kf] * WINO_G[nu][kt] * (double)tap(c, co, ci, kt, kf);
  return u;
}

// DIRECT, conv3x3_mfma: [cg][chunk of CK ci][tap = kt * 3 + kf][ci][COP co] (conv-form taps, zero padded)
static void direct_image(const ConvWeights& c, float* w) {
  const int nchunk = (c.Cin + CK - 1) / CK, COP = c.cop;
  for (int cg = 0; cg < c.ncg; ++cg)
    for (int kc = 0; kc < nchunk; ++kc)
      for (int kt = 0; kt < 3; ++kt)
        for (int kf = 0; kf < 3; ++kf)
          for (int cil = 0; cil < CK; ++cil)
            for (int col = 0; col < COP; ++col) {
              const int ci = kc * CK + cil, co = cg * COP + col;
              w[((((long long)cg * nchunk + kc) * 9 + (kt * 3 + kf)) * CK + cil) * COP + col] =
                  (ci < c.Cin && co < c.Cout) ? tap(c, co, ci, kt, kf) : 0.f;
            }
}

static inline unsigned short f32_to_bf16_rne(float f) {
  unsigned int u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
static inline float bf16_to_f32(unsigned short h) {
  unsigned int u = (unsigned int)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// X6, conv_wprep6_k's source: float32 weights [cg][chunk of 8 ci][tap = kt*3 + kf][32 co][8 ci], zero padded
static void wf6_image(const ConvWeights& c, float* wf) {
  const int nchunk = (c.Cin + 7) / 8;
  const int ncg = (c.Cout + 31) / 32;
  for (int cg = 0; cg < ncg; ++cg)
    for (int kc = 0; kc < nchunk; ++kc)
      for (int kt = 0; kt < 3; ++kt)
        for (int kf = 0; kf < 3; ++kf)
          for (int col = 0; col < 32; ++col)
            for (int e = 0; e < 8; ++e) {
              const int ci = kc * 8 + e, co = cg * 32 + col;
              wf[((((long long)cg * nchunk + kc) * 9 + (kt * 3 + kf)) * 32 + col) * 8 + e] =
                  (ci < c.Cin && co < c.Cout) ? tap(c, co, ci, kt, kf) : 0.f;
            }
}

// X6_FIRST: the first layer's weights as one exact 3-part bf16 image per 8-channel chunk, in conv_wprep6_k's unit order (unit
// ((kf*3 + p)*2 + kt)*32 + co for kt < 2, 576 + (kf*3 + p)*32 + co for kt = 2; 8 channels per unit): w = hi + mid + lo exactly
static void w6s_image(const ConvWeights& c, float* dst) {
  const int nchunk = (c.Cin + 7) / 8;
  unsigned short* img = reinterpret_cast<unsigned short*>(dst);
  for (int kc = 0; kc < nchunk; ++kc)
    for (int kt = 0; kt < 3; ++kt)
      for (int kf = 0; kf < 3; ++kf)
        for (int co = 0; co < 32; ++co)
          for (int e = 0; e < 8; ++e) {
            const int ci = kc * 8 + e;
            const float v = (ci < c.Cin && co < c.Cout) ? tap(c, co, ci, kt, kf) : 0.f;
            const unsigned short h = f32_to_bf16_rne(v);
            const float r1 = v - bf16_to_f32(h);
            const unsigned short m = f32_to_bf16_rne(r1);
            const unsigned short l = f32_to_bf16_rne(r1 - bf16_to_f32(m));
            const unsigned short part[3] = {h, m, l};
            for (int p = 0; p < 3; ++p) {
              const long long unit = kt < 2 ? ((kf * 3 + p) * 2 + kt) * 32 + co : 576 + (kf * 3 + p) * 32 + co;
              img[((long long)kc * 864 + unit) * 8 + e] = part[p];
            }
          }
}

// FEW, conv3x3_few (the <= 4-channel last layer on the vector ALU): [ci][tap = kt * 3 + kf][4 co] conv-form taps, zero padded
static void few_image(const ConvWeights& c, float* img) {
  for (int ci = 0; ci < c.Cin; ++ci)
    for (int kt = 0; kt < 3; ++kt)
      for (int kf = 0; kf < 3; ++kf)
        for (int co = 0; co < 4; ++co) img[((long long)ci * 9 + (kt * 3 + kf)) * 4 + co] = co < c.Cout ? tap(c, co, ci, kt, kf) : 0.f;
}

// W1D, conv3x3_mfma<.., W1D>: U = G g along T per (co, ci, kf), conv-form taps, [cg32][chunk][nu * 3 + kf][ci][32]
static void w1d_image(const ConvWeights& c, float* img) {
  const int nchunk = (c.Cin + CK - 1) / CK, ncg = (c.Cout + 31) / 32;
  for (int cg = 0; cg < ncg; ++cg)
    for (int kc = 0; kc < nchunk; ++kc)
      for (int nu = 0; nu < 4; ++nu)
        for (int kf = 0; kf < 3; ++kf)
          for (int cil = 0; cil < CK; ++cil)
            for (int col = 0; col < 32; ++col) {
              const int ci = kc * CK + cil, co = cg * 32 + col;
              double u = 0.0;
              if (ci < c.Cin && co < c.Cout)
                for (int kt = 0; kt < 3; ++kt) u += WINO_G[nu][kt] * (double)tap(c, co, ci, kt, kf);
              img[((((long long)cg * nchunk + kc) * 12 + (nu * 3 + kf)) * CK + cil) * 32 + col] = (float)u;
            }
}

// WINO, conv3x3_wino_f32: Winograd-domain weights U = G g G^T of a stride-1 same-padded conv, G = [1 0 0; .5 .5 .5; .5 -.5 .5;
// 0 0 1]; position pos = xi * 4 + nu with xi along frequency (kf) and nu along time (kt).  Image order: [cg of 32 co][chunk of
// 8 ci][pos / 4][ci][co][pos % 4], zero padded past Cout.  Computed in double, rounded once.  Signs: positions with nu = 2
// carry a minus because the kernel's packed input transform produces -V there (conv_wino.hip, pk_t23); positions with nu = 3
// and positions with xi = 3 carry one each (both: none) so that the inverse transform A^T M A = sums with a single mixed-sign
// step per row (conv_wino.hip epilogue: the accumulators hold -M there).
static inline bool wino_minus(int xi, int nu) { return (nu == 2) != ((nu == 3) != (xi == 3)); }
static void wino_image(const ConvWeights& c, float* img) {
  const int nchunk = c.Cin / 8, ncg = (c.Cout + 31) / 32;
  for (int cg = 0; cg < ncg; ++cg)
    for (int kc = 0; kc < nchunk; ++kc)
      for (int cil = 0; cil < 8; ++cil)
        for (int col = 0; col < 32; ++col) {
          const int ci = kc * 8 + cil, co = cg * 32 + col;
          for (int pos = 0; pos < 16; ++pos) {
            const int xi = pos >> 2, nu = pos & 3;
            const double u = co < c.Cout ? wino_u(c, co, ci, xi, nu) : 0.0;
            img[(((((long long)cg * nchunk + kc) * 4 + (pos >> 2)) * 8 + cil) * 32 + col) * 4 + (pos & 3)] = (float)(wino_minus(xi, nu) ? -u : u);
          }
        }
}
// ... and of output channels [co0, co0 + 16) for the 16-row body: [chunk of 8 ci][K-step s of 4 ci][pos / 4][ci % 4][16 co][pos % 4],
// the same signs
static void wino_image16(const ConvWeights& c, int co0, float* img) {
  const int nchunk = c.Cin / 8;
  for (int kc = 0; kc < nchunk; ++kc)
    for (int cil = 0; cil < 8; ++cil)
      for (int col = 0; col < 16; ++col) {
        const int ci = kc * 8 + cil, co = co0 + col;
        for (int pos = 0; pos < 16; ++pos) {
          const int xi = pos >> 2, nu = pos & 3;
          const double u = wino_u(c, co, ci, xi, nu);
          const int s = cil >> 2, kk = cil & 3;
          img[((((((long long)kc * 2 + s) * 4 + (pos >> 2)) * 4 + kk) * 16 + col) * 4) + (pos & 3)] = (float)(wino_minus(xi, nu) ? -u : u);
        }
      }
}

// ---- kind -> image ------------------------------------------------------------------------------------------------------------------
long long conv_image_floats(ConvKind k, const ConvWeights& c) {
  const long long g32 = (c.Cout + 31) / 32, k8 = (c.Cin + 7) / 8;
  switch (k) {
    case ConvKind::DIRECT: return (long long)c.ncg * ((c.Cin + CK - 1) / CK) * 9 * CK * c.cop;
    case ConvKind::W1D: return g32 * ((c.Cin + CK - 1) / CK) * 12 * CK * 32;
    case ConvKind::FEW: return (long long)c.Cin * 36;
    case ConvKind::WINO: return conv_wino_ww16_at(c.Cin, c.Cout) + ((c.Cout & 31) == 16 ? (long long)(c.Cin / 8) * 2048 : 0);
    case ConvKind::X6_FIRST: return k8 * 864 * 4;                     // 864 units x 16 bytes = x 4 floats
    case ConvKind::X6: return g32 * k8 * 9 * 32 * 8;
  }
  return 0;
}

void conv_image_pack(ConvKind k, const ConvWeights& c, float* img) {
  switch (k) {
    case ConvKind::DIRECT: direct_image(c, img); break;
    case ConvKind::W1D: w1d_image(c, img); break;
    case ConvKind::FEW: few_image(c, img); break;
    case ConvKind::WINO:
      wino_image(c, img);
      if ((c.Cout & 31) == 16) wino_image16(c, c.Cout - 16, img + conv_wino_ww16_at(c.Cin, c.Cout));
      break;
    case ConvKind::X6_FIRST: w6s_image(c, img); break;
    case ConvKind::X6: wf6_image(c, img); break;
  }
}

}  // namespace mn
