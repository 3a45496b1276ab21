// Which kernel runs a 3x3 conv layer, and which weight image it reads: decided HERE, once per layer and arithmetic mode, when the
// plan is built (net.hip build_plan -> ConvL::kind[]).  misonet_net_commit reserves and packs the images of the kinds that occur,
// run_conv switches on the kind, misonet_net_conv_plan reports it.  Host code only.
//
// A new conv kernel is registered in this file and nowhere else in the dispatch: a ConvKind, its `*_ok` predicate (defined in the
// kernel's own file beside the limits it depends on, and used by its launcher as the guard), its line in conv_select(), and its
// weight image in conv_weights.hip (conv_image_floats / conv_image_pack).
#pragma once
#include "kernels.hpp"

// Arithmetic modes: 0 "f32", 3 "bf16x6", 5 "f32w".  The numbers 1, 2 (bf16x3), 4 (f16x3) and 6 (bf16x6w) belonged to alternatives that
// were measured and dropped (LAB.md, "Leftovers of the experiment build"); the library answers MISONET_EINVAL to them.

namespace mn {

constexpr int CONV_NMODES = 6;                    // ConvL::kind[] is indexed by the mode number, 0 ... 5
inline bool conv_mode_built(int mode) { return mode == 0 || mode == 3 || mode == 5; }

// the values are ABI: misonet_net_conv_plan (include/misonet.h) reports them
enum class ConvKind : int {
  DIRECT = 0,    // conv3x3_mfma (conv.hip): every shape; the exact f32 kernel
  W1D,           // conv3x3_mfma<.., W1D> (conv.hip): 1-D Winograd along T, the layers outside the dense blocks in f32w
  FEW,           // conv3x3_few (conv_few.hip): 2 / 4 output channels without activation on the vector ALU
  WINO,          // conv3x3_wino_f32 (conv_wino.hip): Winograd F(2x2, 3x3), the DenseBlock convs in f32w
  X6_FIRST,      // conv3x3_x6_first (conv_bf16x6.hip): the network's first layer, planar float32 in, oct3 out
  X6,            // conv_wprep6_k + conv3x3_bf16x6 (conv_bf16x6.hip): oct3 in
};
constexpr int CONV_NKIND = 6;

// What a kernel's eligibility depends on: static per layer and mode, nothing of T, N or a pointer.
struct ConvShape {
  int Cin, Cout, Fin, Fout;
  int sf, padf, tr2, act;
  bool transposed;            // ConvTranspose2d (conv form: flipped taps, padf == 2)
  int ident_c;                // input channels [0, ident_c) are consumed un-normalised
  bool net_input;             // the input buffer is the network input
  int in_oct, out_oct;        // ConvArgs::in_oct / out_oct layout codes
};
// the shape a launcher sees (a conv-form padding of 2 exists only for transposed layers: ConvArgs::padf)
inline ConvShape conv_shape(const ConvArgs& a, bool net_input = false) {
  return {a.Cin, a.Cout, a.Fin, a.Fout, a.sf, a.padf, a.tr2, a.act, a.padf == 2, a.ident_c, net_input, a.in_oct, a.out_oct};
}

// eligibility, each beside its kernel; launch_conv_<kind> refuses (hipErrorInvalidValue) what its predicate refuses
bool conv_w1d_ok(const ConvShape& s);        // conv.hip
bool conv_few_ok(const ConvShape& s);        // conv_few.hip
bool conv_wino_ok(const ConvShape& s);       // conv_wino.hip
bool conv_x6_first_ok(const ConvShape& s);   // conv_bf16x6.hip

// The kernel of a layer in precision mode `mode`; s.in_oct / s.out_oct are that mode's layouts of the layer's buffers.  First match
// wins.  The oct3 layout leaves no choice (only its own kernel reads it); a first layer of bf16x6 that conv3x3_x6_first does not take
// runs on the exact f32 kernel.
inline ConvKind conv_select(const ConvShape& s, int mode) {
  const bool planar = mode == 0 || mode == 5;                   // every buffer planar float32
  if (s.out_oct == 3 && conv_x6_first_ok(s)) return ConvKind::X6_FIRST;
  if (s.in_oct == 3) return ConvKind::X6;
  if (planar && conv_few_ok(s)) return ConvKind::FEW;
  if (mode == 5 && conv_wino_ok(s)) return ConvKind::WINO;
  if (mode == 5 && conv_w1d_ok(s)) return ConvKind::W1D;
  return ConvKind::DIRECT;
}

// ---- weight images (conv_weights.hip) ---------------------------------------------------------------------------------------------
struct ConvWeights {
  const float* W;             // Conv2d [Cout][Cin][3][3] or ConvTranspose2d [Cin][Cout][3][3]
  int Cin, Cout;
  bool transposed;
  int cop, ncg;               // DIRECT only: output channels per group (32 / 64) and groups
};
// floats the image of `k` takes in the weight arena (a multiple of 64 is not required; 0: the kind reads no image of its own)
long long conv_image_floats(ConvKind k, const ConvWeights& c);
void conv_image_pack(ConvKind k, const ConvWeights& c, float* img);
// WINO: the image of the last 16 output channels of a layer with Cout % 32 == 16 (ConvArgs::ww16) lies behind the main image
inline long long conv_wino_ww16_at(int Cin, int Cout) { return (long long)((Cout + 31) / 32) * (Cin / 8) * 16 * 8 * 32; }

}  // namespace mn
