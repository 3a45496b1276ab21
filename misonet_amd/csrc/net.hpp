// The network object behind misonet_net_* and what the fused pipeline (api_pipeline.hip) needs of it: the plan, the workspace
// layout and the forward.  Defined in net.hip.  Host code only.
#pragma once
#include "conv_select.hpp"
#include "api_common.hpp"

#include <string>

namespace mn {

struct Tensor {
  std::string name;
  long long numel;
  std::vector<float> host;
  bool set = false;
};

enum { B_IN = 0, B_E0, B_E1, B_E2, B_E3, B_E4, B_D0, B_D1, B_D2, B_D3, B_D4, B_D5, B_D6, B_X2, B_X3, B_X4, B_X5, B_X6,
       B_OUT, B_TXA, B_TXB, B_TD, B_TP, NBUF };

struct BufSpec { int C = 0, F = 0; };

struct ConvL {
  int in_buf, in_c0, Cin, ident_c;
  int out_buf, out_c0, Cout;
  int sf, padf, tr2, act;
  bool transposed;
  int wt, bt;                   // tensor indices
  int cop, ncg;
  ConvKind kind[CONV_NMODES];       // the layer's kernel per precision mode (conv_select.hpp), filled by build_plan
  long long img_off[CONV_NKIND];    // commit: offset (floats) into the device weight arena of the image of each kind that occurs in
                                    // kind[] (and of DIRECT, always); -1: not packed
  long long b_off = 0;              // ... and of the bias [ncg * cop]
  const float* img(const float* w_dev, ConvKind k) const { return w_dev + img_off[(int)k]; }
};

struct TcnHalf {
  int dw, prelu, gamma, beta, pw; long long o_dw, o_prelu, o_gamma, o_beta, o_pw;
  // the OUTER norm in front of this half (model.py:530,535; cfg.tcn_norm): tensors (gLN / cLN: gamma, beta; BatchNorm1d:
  // weight, bias, running_mean, running_var) and the per-channel (scale, shift) pair the kernels read
  int on[4] = {-1, -1, -1, -1};
  long long o_nsc = 0, o_nsh = 0;
};
struct TcnBlock { int dilation; TcnHalf h[2]; };

struct Tap { std::string name; int buf, c0, C; bool normalised; };

struct Layout {
  int N, T, Tp;
  long long data_off[NBUF];      // floats: activation buffers (b < B_TXA): offset INSIDE a sample's block of the arena (sample n
                                 // at + n * sample_stride); TCN buffers: offset of the whole [N][128][Tp] block
  long long sample_stride;       // floats per sample of the activation arena
  long long in_ext_off = -1;     // >= 0: the network input lives OUTSIDE this workspace, at ws + in_ext_off bytes, with
  long long in_ext_bstride = 0;  // in_ext_bstride floats between samples (the pipeline's MISO3 input, see pipe_layout)
  long long stats_off[NBUF];     // 8-byte words (dstat_t): [N][C][2][DS_NL] per buffer
  long long tcn_xs, tcn_ps, tcn_gln;   // words (2 per double2 partial): [15][N*128*slots], [14][N*128*slots], [28][N*32]
  long long stats_doubles;       // words in all
  long long data_base;           // bytes from ws start to the float arena
  long long wps_base, wps_nstride;   // bytes: per-sample folded weights of the layer in flight (DMA dataflow)
  long long btab_base, btab_nstride; // bytes / floats: per-sample border-aware shift table
  long long fstat_base;              // bytes: [N][Tp] float2 per-frame (mean, rstd) of the cLN outer norm (cfg.tcn_norm == 2)
  long long total_bytes;
};

}  // namespace mn

struct misonet_net {
  misonet_cfg cfg;
  int S;                         // speakers out = out_ch / 2
  mn::BufSpec bufs[mn::NBUF];
  std::vector<mn::Tensor> tensors;
  std::vector<mn::ConvL> enc, dec;
  std::vector<mn::TcnBlock> tcn;
  std::vector<mn::Tap> taps;
  float* w_dev = nullptr;
  bool committed = false;
  bool keep_taps = false;        // true: no buffer shares memory with another (every tap stays readable after a forward)
  int precision = 3;             // 0: exact f32 MFMA, 3: bf16x6 DMA dataflow (the default: fp32-faithful, what bench.py reports),
                                 // 5: f32 MFMA with the dense-block convs in Winograd F(2x2, 3x3) form ("f32w": planar float32
                                 // layout like mode 0); conv_select.hpp conv_mode_built
};

namespace mn {

inline long long align_up(long long x, long long a) { return (x + a - 1) / a * a; }

Layout make_layout(const misonet_net* n, int N, int T, bool ext_in = false);
// floats between consecutive samples of buffer b: the activation arena is SAMPLE-major (all buffers of a sample in one
// block, so that buffers whose lifetimes do not overlap can share memory: make_layout), the TCN buffers are buffer-major
long long bstride(const misonet_net* n, const Layout& L, int b);
inline float* buf_ptr(const Layout& L, void* ws, int b) {
  if (b == B_IN && L.in_ext_off >= 0) return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + L.in_ext_off);
  return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + L.data_base) + L.data_off[b];
}
// IN buffer already filled (planar).  Leaves the result (raw) in B_OUT.
int forward_planar(misonet_net* n, const Layout& L, void* ws, hipStream_t s);

}  // namespace mn
