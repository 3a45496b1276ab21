// The network of libmisonet_hip.so: layer plan of a MISO trunk (reference model.py:8-111 / 282-395), the weight arena (the
// images themselves: conv_weights.hip), workspace layout and forward scheduling, behind the misonet_net_* entry points of
// include/misonet.h.  Also the library's runtime: the error report, per-launch profiling and events.  The rest of the C ABI lies in
// one host file per domain: api_frontend.hip (STFT / iSTFT), api_array.hip (beamformers, WPE, PIT, continuous separation),
// api_score.hip (scores, BSS-eval, STOI) and api_pipeline.hip (the fused pipeline); what they share: api_common.hpp, net.hpp.
#include "net.hpp"

#include <math.h>
#include <cmath>
#include <algorithm>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace mn;

static thread_local char g_err[512] = "";       // the one message buffer: only fail() writes it, only misonet_last_error reads it
int mn::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

Prof mn::g_profs[MAX_DEV];
std::atomic<int> mn::g_prof_any{0};

// ---------------------------------------------------------------------------------------------------------------
static int find_tensor(const misonet_net* n, const std::string& name) {
  for (size_t i = 0; i < n->tensors.size(); ++i)
    if (n->tensors[i].name == name) return (int)i;
  return -1;
}
static int add_tensor(misonet_net* n, const std::string& name, long long numel) {
  Tensor t;
  t.name = name;
  t.numel = numel;
  n->tensors.push_back(t);
  return (int)n->tensors.size() - 1;
}

static ConvL make_conv(misonet_net* n, const std::string& prefix, int in_buf, int in_c0, int Cin, int ident_c, int out_buf,
                       int out_c0, int Cout, int sf, int padf, bool transposed, int act) {
  ConvL L;
  L.in_buf = in_buf; L.in_c0 = in_c0; L.Cin = Cin; L.ident_c = ident_c;
  L.out_buf = out_buf; L.out_c0 = out_c0; L.Cout = Cout;
  L.transposed = transposed;
  L.act = act;
  std::fill(L.img_off, L.img_off + CONV_NKIND, -1LL);
  if (transposed) {
    L.tr2 = (sf == 2);
    L.sf = 1;
    L.padf = 2;          // stride-1 transposed conv == conv with flipped taps and full padding
  } else {
    L.tr2 = 0; L.sf = sf; L.padf = padf;
  }
  L.wt = add_tensor(n, prefix + ".weight", (long long)Cin * Cout * 9);
  L.bt = add_tensor(n, prefix + ".bias", Cout);
  L.cop = L.tr2 ? 32 : conv_cop(Cout);       // (conv3x3_mfma runs two output rows per wave on the stride-2 transposed layers)
  L.ncg = (Cout + L.cop - 1) / L.cop;
  return L;
}

// DenseBlock(init_ch, g1, g2) on buffer `buf` ([x | y0..y3]); y4 -> (out_buf, out_c0)   (model.py:437-482)
static void add_dense(misonet_net* n, std::vector<ConvL>& v, const std::string& prefix, int buf, int init_ch, int g1, int g2,
                      int ident_c, int out_buf, int out_c0) {
  for (int i = 0; i < 5; ++i) {
    const int cin = init_ch + i * g1;
    char nm[64];
    snprintf(nm, sizeof(nm), ".conv%d.0", i + 1);
    if (i < 4)
      v.push_back(make_conv(n, prefix + nm, buf, 0, cin, ident_c, buf, cin, g1, 1, 1, false, 1));
    else
      v.push_back(make_conv(n, prefix + nm, buf, 0, cin, ident_c, out_buf, out_c0, g2, 1, 1, false, 1));
  }
}

// precision 3 ("bf16x6"), the DMA dataflow: every buffer between the network input and its output travels in the oct3 layout (3
// bf16 parts = 6 bytes per element) -- the dense-block buffers and what lies between them, and the F <= 3 bottleneck buffers D0 / D1
// (the TCN reads / writes the layout at its two ends), so that encoder 6 and decoders 0-1 run on the persistent kernel too.  The
// network input / output and the TCN stay planar float32.  Returns the ConvArgs::in_oct / out_oct code.
static inline int buf_oct(int precision, int b) {
  if (precision != 3) return 0;
  return ((b >= B_E0 && b <= B_E4) || (b >= B_D0 && b <= B_D6) || (b >= B_X2 && b <= B_X6)) ? 3 : 0;
}
static inline int buf_oct(const misonet_net* n, int b) { return buf_oct(n->precision, b); }

static int freq_after_conv(int F, int sf) { return (F - 3) / sf + 1; }

static int build_plan(misonet_net* n) {
  const misonet_cfg& c = n->cfg;
  if (c.n_freq != 129) return fail(MISONET_EINVAL, "n_freq must be 129 (got %d): the encoder must reduce F to one bin", c.n_freq);
  if (c.tcn_norm < 0 || c.tcn_norm > 3)
    return fail(MISONET_EINVAL, "tcn_norm must be 0 (IN), 1 (gLN), 2 (cLN) or 3 (BatchNorm1d, eval) (got %d)", c.tcn_norm);
  if (c.in_ch < 2 || c.in_ch % 2 || c.out_ch < 2 || c.out_ch % 2 || c.in_ch > 64 || c.out_ch > 32)
    return fail(MISONET_EINVAL, "in_ch/out_ch must be even and small (got %d/%d)", c.in_ch, c.out_ch);
  for (int i = 0; i < 7; ++i) {
    if (c.en_ch[i] <= 0 || c.en_ch[i] % 8 || c.de_ch[i] <= 0 || c.de_ch[i] % 8)
      return fail(MISONET_EINVAL, "bottleneck channels must be positive multiples of 8");
    if (c.en_ch[6 - i] != c.de_ch[i])
      return fail(MISONET_EINVAL, "U-Net skip concat needs en_ch[6-i] == de_ch[i] (model.py:35,99)");
  }
  if (c.en_ch[6] != 128) return fail(MISONET_EINVAL, "the TCN is TemporalConvNet(2,7,128,128,128) (model.py:31): en_ch[6] must be 128");
  for (int i = 0; i < 7; ++i)
    if (c.en_ch[i] > 128) return fail(MISONET_EINVAL, "channel counts above 128 are not supported");
  n->S = c.out_ch / 2;
  const int* en = c.en_ch;
  const int* de = c.de_ch;
  // frequency sizes per encoder level (model.py:40-54): F_e[b] = output bins of encoder b
  int Fe[7];
  Fe[0] = freq_after_conv(c.n_freq, 1);
  for (int b = 1; b < 7; ++b) Fe[b] = freq_after_conv(Fe[b - 1], b == 6 ? 1 : 2);
  if (Fe[6] != 1) return fail(MISONET_EINVAL, "encoder does not reduce to one frequency bin");
  // buffers
  n->bufs[B_IN] = {c.in_ch, c.n_freq};
  for (int b = 0; b < 5; ++b) n->bufs[B_E0 + b] = {5 * en[b], Fe[b]};
  n->bufs[B_D0] = {2 * de[0], Fe[6]};
  n->bufs[B_D1] = {2 * de[1], Fe[5]};
  for (int i = 2; i < 7; ++i) {
    n->bufs[B_D0 + i] = {6 * de[i], Fe[6 - i]};
    n->bufs[B_X2 + (i - 2)] = {2 * de[i], Fe[6 - i]};
  }
  n->bufs[B_OUT] = {c.out_ch, c.n_freq};
  for (int b = B_TXA; b <= B_TP; ++b) n->bufs[b] = {128, 1};

  // ---- encoders (model.py:40-54); xs[b] is written straight into decoder buffer D[6-b] at channel de[6-b] ----
  char nm[96];
  for (int b = 0; b < 7; ++b) {
    const int skip_buf = B_D0 + (6 - b), skip_c0 = de[6 - b];
    const int src_buf = (b == 0) ? B_IN : B_D0 + (7 - b);
    const int src_c0 = (b == 0) ? 0 : de[7 - b];
    const int cin = (b == 0) ? c.in_ch : en[b - 1];
    if (b == 0) {
      n->enc.push_back(make_conv(n, "encoders.0.0.conv2d", B_IN, 0, cin, cin, B_E0, 0, en[0], 1, 0, false, 0));
      add_dense(n, n->enc, "encoders.0.1", B_E0, en[0], en[0], en[0], en[0], skip_buf, skip_c0);
    } else if (b < 5) {
      snprintf(nm, sizeof(nm), "encoders.%d.0.net.0", b);
      n->enc.push_back(make_conv(n, nm, src_buf, src_c0, cin, 0, B_E0 + b, 0, en[b], 2, 0, false, 1));
      snprintf(nm, sizeof(nm), "encoders.%d.1", b);
      add_dense(n, n->enc, nm, B_E0 + b, en[b], en[b], en[b], 0, skip_buf, skip_c0);
    } else {
      snprintf(nm, sizeof(nm), "encoders.%d.0.net.0", b);
      n->enc.push_back(make_conv(n, nm, src_buf, src_c0, cin, 0, skip_buf, skip_c0, en[b], b == 6 ? 1 : 2, 0, false, 1));
    }
  }
  // ---- decoders (model.py:56-73) ----
  for (int i = 0; i < 7; ++i) {
    const int buf = B_D0 + i;
    const int cin = 2 * de[i];
    const int cout = (i == 6) ? c.out_ch : de[i + 1];
    const int obuf = (i == 6) ? B_OUT : B_D0 + i + 1;
    if (i >= 2) {
      snprintf(nm, sizeof(nm), "decoders.%d.0", i);
      add_dense(n, n->dec, nm, buf, cin, cin / 2, cin, 0, B_X2 + (i - 2), 0);
      snprintf(nm, sizeof(nm), i == 6 ? "decoders.%d.1.deconv2d" : "decoders.%d.1.net.0", i);
      n->dec.push_back(make_conv(n, nm, B_X2 + (i - 2), 0, cin, 0, obuf, 0, cout, i == 6 ? 1 : 2, 0, true, i == 6 ? 0 : 1));
    } else {
      snprintf(nm, sizeof(nm), "decoders.%d.0.net.0", i);
      // decoder 0 consumes [TCN output (raw, identity) | xs[6] (instance-normalised)]
      n->dec.push_back(make_conv(n, nm, buf, 0, cin, i == 0 ? de[0] : 0, obuf, 0, cout, i == 0 ? 1 : 2, 0, true, 1));
    }
  }
  // ---- TCN (model.py:486-567) ----
  for (int r = 0; r < 2; ++r)
    for (int x = 0; x < 7; ++x) {
      TcnBlock tb;
      tb.dilation = 1 << x;
      for (int h = 0; h < 2; ++h) {
        if (c.tcn_norm) {                          // state_dict order: the norm module precedes its DepthwiseSeparableConv
          snprintf(nm, sizeof(nm), "TCN.temporal_conv_net.%d.%d.net.%d", r, x, h == 0 ? 0 : 3);
          const std::string q(nm);
          if (c.tcn_norm == 3) {
            tb.h[h].on[0] = add_tensor(n, q + ".weight", 128);
            tb.h[h].on[1] = add_tensor(n, q + ".bias", 128);
            tb.h[h].on[2] = add_tensor(n, q + ".running_mean", 128);
            tb.h[h].on[3] = add_tensor(n, q + ".running_var", 128);
          } else {
            tb.h[h].on[0] = add_tensor(n, q + ".gamma", 128);
            tb.h[h].on[1] = add_tensor(n, q + ".beta", 128);
          }
        }
        snprintf(nm, sizeof(nm), "TCN.temporal_conv_net.%d.%d.net.%d.net", r, x, h == 0 ? 2 : 5);
        const std::string p(nm);
        tb.h[h].dw = add_tensor(n, p + ".0.weight", 128 * 3);
        tb.h[h].prelu = add_tensor(n, p + ".1.weight", 1);
        tb.h[h].gamma = add_tensor(n, p + ".2.gamma", 128);
        tb.h[h].beta = add_tensor(n, p + ".2.beta", 128);
        tb.h[h].pw = add_tensor(n, p + ".3.weight", 128 * 128);
      }
      n->tcn.push_back(tb);
    }
  // ---- taps ----
  n->taps.push_back({"enc0_conv", B_E0, 0, en[0], false});
  for (int b = 0; b < 7; ++b) {
    snprintf(nm, sizeof(nm), "enc%d", b);
    n->taps.push_back({nm, B_D0 + (6 - b), de[6 - b], en[b], true});
  }
  n->taps.push_back({"tcn_out", B_D0, 0, 128, false});
  for (int i = 0; i < 6; ++i) {
    snprintf(nm, sizeof(nm), "dec%d", i);
    n->taps.push_back({nm, B_D0 + i + 1, 0, de[i + 1], true});
  }
  n->taps.push_back({"dec6", B_OUT, 0, c.out_ch, false});
  // ---- the kernel of every conv layer in every arithmetic mode ----
  for (std::vector<ConvL>* v : {&n->enc, &n->dec})
    for (ConvL& l : *v)
      for (int mode = 0; mode < CONV_NMODES; ++mode) {
        const ConvShape sh = {l.Cin, l.Cout, n->bufs[l.in_buf].F, n->bufs[l.out_buf].F, l.sf, l.padf, l.tr2, l.act, l.transposed,
                              l.ident_c, l.in_buf == B_IN, buf_oct(mode, l.in_buf), buf_oct(mode, l.out_buf)};
        l.kind[mode] = conv_mode_built(mode) ? conv_select(sh, mode) : ConvKind::DIRECT;
      }
  return MISONET_OK;
}

// floats one sample occupies in buffer b (an oct3 buffer holds 1.5 floats per element; C is a multiple of 8 there)
static inline long long buf_floats(const misonet_net* n, int Tp, int b) {
  const long long e = (long long)n->bufs[b].C * n->bufs[b].F * Tp;
  return buf_oct(n, b) == 3 ? e + e / 2 : e;
}
long long mn::bstride(const misonet_net* n, const Layout& L, int b) {
  if (b == B_IN && L.in_ext_off >= 0) return L.in_ext_bstride;
  return b >= B_TXA ? buf_floats(n, L.Tp, b) : L.sample_stride;
}

// Lifetime of an activation buffer in steps of a forward: 0 = input written (pack / MISO3 input assembly), 1 + b =
// encoder b, 8 = TCN, 9 + i = decoder i, 16 = results read (unpack; the pipeline also reads MISO1's input and output
// planes after the forward: PIT, MVDR, MISO3 input assembly).  The only cross-level lifetime of the reference is the
// skip list xs (model.py:84-99): decoder buffer D[i] receives xs[6 - i] at encoder 6 - i and is consumed by decoder i;
// an encoder's dense-block buffer E[b] is dead once its last conv has written xs[b], X[i] lives inside decoder i.
static void buf_lifetime(int b, int& t0, int& t1) {
  if (b == B_IN) { t0 = 0; t1 = 16; }
  else if (b >= B_E0 && b <= B_E4) { t0 = t1 = 1 + (b - B_E0); }
  else if (b >= B_D0 && b <= B_D6) { const int i = b - B_D0; t0 = 7 - i; t1 = 9 + i; }
  else if (b >= B_X2 && b <= B_X6) { t0 = t1 = 9 + 2 + (b - B_X2); }
  else { t0 = 15; t1 = 16; }                                     // B_OUT
}

Layout mn::make_layout(const misonet_net* n, int N, int T, bool ext_in) {
  Layout L;
  L.N = N; L.T = T; L.Tp = frames_pitch(T);
  long long so = 0;
  for (int b = 0; b < NBUF; ++b) {
    L.stats_off[b] = so;
    so += (long long)N * n->bufs[b].C * 2 * DS_NL;
  }
  const long long tslots = tcn_part_slots(T);          // TCN statistics: plain double2 partials (tcn.hip), never zeroed
  so = (so + 1) & ~1LL;                                // 16-byte alignment of the double2 arrays
  L.tcn_xs = so;  so += 15LL * N * 128 * tslots * 2;
  L.tcn_ps = so;  so += 14LL * N * 128 * tslots * 2;
  L.tcn_gln = so; so += 28LL * N * 32 * 2;
  L.stats_doubles = so;
  L.data_base = align_up(256 + so * 8, 256);
  // ---- activation arena: per-sample offsets by first fit over (lifetime x address) rectangles, largest buffer first ----
  {
    struct Rect { int b, t0, t1; long long off, size; };
    std::vector<Rect> placed;
    std::vector<int> order;
    for (int b = 0; b < B_TXA; ++b)
      if (!(ext_in && b == B_IN)) order.push_back(b);          // an external input takes no room in the arena
    L.data_off[B_IN] = 0;
    std::sort(order.begin(), order.end(), [&](int x, int y) {
      const long long sx = buf_floats(n, L.Tp, x), sy = buf_floats(n, L.Tp, y);
      return sx != sy ? sx > sy : x < y;
    });
    long long top = 0;
    for (int b : order) {
      Rect r;
      r.b = b;
      r.size = align_up(buf_floats(n, L.Tp, b), 64);
      buf_lifetime(b, r.t0, r.t1);
      if (n->keep_taps) { r.t0 = 0; r.t1 = 16; }
      // candidate offsets: 0 and the end of every placed rectangle that is alive at the same time
      std::vector<long long> cand(1, 0);
      for (const Rect& q : placed)
        if (q.t0 <= r.t1 && r.t0 <= q.t1) cand.push_back(q.off + q.size);
      std::sort(cand.begin(), cand.end());
      for (long long o : cand) {
        bool ok = true;
        for (const Rect& q : placed)
          if (q.t0 <= r.t1 && r.t0 <= q.t1 && o < q.off + q.size && q.off < o + r.size) { ok = false; break; }
        if (ok) { r.off = o; break; }
      }
      placed.push_back(r);
      L.data_off[b] = r.off;
      top = std::max(top, r.off + r.size);
    }
    L.sample_stride = top;
  }
  long long d = (long long)N * L.sample_stride;
  for (int b = B_TXA; b < NBUF; ++b) {
    L.data_off[b] = d;
    d += align_up((long long)N * buf_floats(n, L.Tp, b), 64);
  }
  long long wmax = 0, cmax = 0;
  auto scan = [&](const std::vector<ConvL>& v) {
    for (const ConvL& c : v) {
      wmax = std::max(wmax, conv_bf16x6_wps_bytes((c.Cin + 7) / 8 * 8, c.Cout));
      cmax = std::max(cmax, (c.Cout + 31) / 32 * 32LL);
    }
  };
  scan(n->enc); scan(n->dec);
  L.wps_base = align_up(L.data_base + d * 4, 256);
  L.wps_nstride = wmax;
  L.btab_base = align_up(L.wps_base + wmax * N, 256);
  L.btab_nstride = cmax * 9 * 4;                    // up to 4 shares of the shift table (conv_wprep6_k)
  L.fstat_base = align_up(L.btab_base + L.btab_nstride * 4 * N, 256);
  L.total_bytes = L.fstat_base + (n->cfg.tcn_norm == 2 ? (long long)N * L.Tp * 8 : 0);
  return L;
}

static inline dstat_t* stats_base(void* ws) { return reinterpret_cast<dstat_t*>(reinterpret_cast<char*>(ws) + 256); }
static inline dstat_t* stats_ptr(const Layout& L, void* ws, int b) { return stats_base(ws) + L.stats_off[b]; }

// launch layer c on all samples with the kernel the plan chose for the current mode (ConvL::kind)
static int run_conv(const misonet_net* n, const Layout& L, void* ws, const ConvL& c, hipStream_t s) {
  const ConvKind kind = c.kind[n->precision];
  const int nb = L.N;
  ConvArgs a = {};
  a.in_bstride = bstride(n, L, c.in_buf);
  a.out_bstride = bstride(n, L, c.out_buf);
  a.in_sstride = n->bufs[c.in_buf].C;
  a.out_sstride = n->bufs[c.out_buf].C;
  a.in = buf_ptr(L, ws, c.in_buf);
  a.out = buf_ptr(L, ws, c.out_buf);
  a.in_stats = stats_ptr(L, ws, c.in_buf);
  a.out_stats = stats_ptr(L, ws, c.out_buf);
  a.bias = n->w_dev + c.b_off;
  a.in_c0 = c.in_c0; a.Cin = c.Cin; a.Fin = n->bufs[c.in_buf].F; a.ident_c = c.ident_c;
  a.out_c0 = c.out_c0; a.Cout = c.Cout; a.Fout = n->bufs[c.out_buf].F;
  a.T = L.T; a.Tp = L.Tp;
  a.sf = c.sf; a.padf = c.padf; a.tr2 = c.tr2; a.act = c.act;
  a.in_oct = buf_oct(n, c.in_buf);
  a.out_oct = buf_oct(n, c.out_buf);
  // output-channel groups: the plan's 32 or 64 channels on the direct kernel, 32 on every other (some of which regroup: conv_select.hpp)
  a.cop = kind == ConvKind::DIRECT ? c.cop : 32;
  a.ncg = (c.Cout + a.cop - 1) / a.cop;
  a.wscale = a.descale = 1.f;
  // the oct3-input kernel reads per-sample weights with the input's instance norm folded in: its prep kernel runs first
  auto prep = [&]() {
    a.wps = reinterpret_cast<char*>(ws) + L.wps_base;
    a.wps_nstride = L.wps_nstride;
    a.btab = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + L.btab_base);
    a.btab_nstride = L.btab_nstride;
    ProfScope pw(s, PK_OTHER);                                     // its own kind: part of the step, not of the conv kernel
    return launch_conv_wprep6(a, c.img(n->w_dev, kind), nb, s);
  };
  hipError_t e = hipSuccess;
  switch (kind) {
    case ConvKind::DIRECT: { a.w = c.img(n->w_dev, kind); ProfScope ps(s, PK_CONV); e = launch_conv(a, nb, s); } break;
    case ConvKind::W1D: { a.w1d = c.img(n->w_dev, kind); ProfScope ps(s, PK_CONV); e = launch_conv_w1d(a, nb, s); } break;
    case ConvKind::FEW: { a.wsm = c.img(n->w_dev, kind); ProfScope ps(s, PK_CONV); e = launch_conv_few(a, nb, s); } break;
    case ConvKind::WINO: {
      a.ww = c.img(n->w_dev, kind);
      if ((c.Cout & 31) == 16) a.ww16 = a.ww + conv_wino_ww16_at(c.Cin, c.Cout);
      ProfScope ps(s, PK_CONV);
      e = launch_conv_wino(a, nb, s);
    } break;
    case ConvKind::X6_FIRST: { ProfScope ps(s, PK_CONV); e = launch_conv_x6_first(a, c.img(n->w_dev, kind), nb, s); } break;
    case ConvKind::X6:
      e = prep();
      if (e == hipSuccess) { ProfScope ps(s, PK_CONV); e = launch_conv_bf16x6(a, nb, s); }
      break;
    default: e = hipErrorInvalidValue; break;
  }
  // a launcher that refuses the layer its kind was chosen for: the selector and the kernel disagree -- never a silent fall-back
  if (e == hipErrorInvalidValue)
    return fail(MISONET_EINVAL, "conv kernel kind %d refuses the layer Cin=%d Cout=%d Fin=%d Fout=%d sf=%d padf=%d tr2=%d act=%d in_oct=%d out_oct=%d (mode %d)",
                (int)kind, a.Cin, a.Cout, a.Fin, a.Fout, a.sf, a.padf, a.tr2, a.act, a.in_oct, a.out_oct, n->precision);
  HIPCHK(e);
  return MISONET_OK;
}

// The workspace header (256 bytes): word 0 = NaN flag; word 2 = LAYOUT STAMP of the forward that last ran in it -- which
// buffer plan (shared arena or one memory per buffer), arithmetic mode and geometry the offsets inside belong to.
// misonet_net_tap compares it before it reads a buffer (a tap after keep_activations(net, 1) on a workspace whose
// forward ran with the SHARED plan passed the old host-side check and read past the smaller workspace).
static unsigned layout_stamp(const misonet_net* n, const Layout& L) {
  unsigned h = 2166136261u;
  auto mix = [&](unsigned long long v) { for (int i = 0; i < 8; ++i) { h ^= (unsigned)(v & 0xff); h *= 16777619u; v >>= 8; } };
  mix(n->keep_taps ? 1 : 0); mix((unsigned)n->precision); mix((unsigned)L.N); mix((unsigned)L.T); mix((unsigned long long)L.total_bytes);
  return h | 1u;                                  // never 0 (= "no forward has run here")
}

int mn::forward_planar(misonet_net* n, const Layout& L, void* ws, hipStream_t s) {
  // the nan flag + the conv statistics (integer limbs are ACCUMULATED); the TCN partial arrays behind them are plainly written
  HIPCHK(hipMemsetAsync(ws, 0, (size_t)(256 + L.tcn_xs * 8), s));
  HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<char*>(ws) + 8), (int)layout_stamp(n, L), 1, s));
  auto run_stack = [&](const std::vector<ConvL>& v) -> int {
    for (const ConvL& c : v) { int r = run_conv(n, L, ws, c, s); if (r) return r; }
    return MISONET_OK;
  };
  { int r = run_stack(n->enc); if (r) return r; }
  // ---- TCN ----
  {
    ProfScope ps_tcn(s, PK_TCN);
    const int N = L.N, T = L.T, Tp = L.Tp;
    double2* xs = reinterpret_cast<double2*>(stats_base(ws) + L.tcn_xs);
    double2* ps = reinterpret_cast<double2*>(stats_base(ws) + L.tcn_ps);
    double2* gl = reinterpret_cast<double2*>(stats_base(ws) + L.tcn_gln);
    const int tslots = tcn_part_slots(T);
    const long long per = (long long)N * 128 * tslots;
    const long long gper = (long long)N * 32;
    float* xa = buf_ptr(L, ws, B_TXA);
    float* xb = buf_ptr(L, ws, B_TXB);
    float* td = buf_ptr(L, ws, B_TD);
    float* tp = buf_ptr(L, ws, B_TP);
    const int skip_c0 = n->cfg.de_ch[0];
    HIPCHK(launch_tcn_prepare(buf_ptr(L, ws, B_D0), bstride(n, L, B_D0), skip_c0, stats_ptr(L, ws, B_D0),
                              n->bufs[B_D0].C, xa, xs, 128, T, Tp, N, s, buf_oct(n, B_D0) == 3));
    float* cur = xa;
    float* nxt = xb;
    const int tcn_x6 = n->precision == 3;     // bf16x6 mode: the point-wise convs in the same arithmetic as the 3x3 convs
    for (int k = 0; k < 14; ++k) {
      const TcnBlock& tb = n->tcn[k];
      const float* W = n->w_dev;
      const int nk = n->cfg.tcn_norm;
      float2* fstat = reinterpret_cast<float2*>(reinterpret_cast<char*>(ws) + L.fstat_base);
      if (nk == 2) HIPCHK(launch_tcn_cln_stats(cur, fstat, 128, T, Tp, N, s));
      HIPCHK(launch_tcn_dw(cur, xs + k * per, k == 0 ? 1 : tslots, W + tb.h[0].o_dw, W + tb.h[0].o_prelu, td, gl + (2 * k) * gper,
                           128, T, Tp, tb.dilation, N, s, nk, W + tb.h[0].o_nsc, W + tb.h[0].o_nsh, fstat));
      HIPCHK(launch_tcn_pw(td, gl + (2 * k) * gper, W + tb.h[0].o_gamma, W + tb.h[0].o_beta, W + tb.h[0].o_pw,
                           nullptr, tp, 128LL * Tp, 0, ps + k * per, 128, T, Tp, N, s, 0, tcn_x6));
      if (nk == 2) HIPCHK(launch_tcn_cln_stats(tp, fstat, 128, T, Tp, N, s));
      HIPCHK(launch_tcn_dw(tp, ps + k * per, tslots, W + tb.h[1].o_dw, W + tb.h[1].o_prelu, td,
                           gl + (2 * k + 1) * gper, 128, T, Tp, tb.dilation, N, s, nk, W + tb.h[1].o_nsc, W + tb.h[1].o_nsh, fstat));
      const bool last = (k == 13);
      float* y = last ? buf_ptr(L, ws, B_D0) : nxt;
      HIPCHK(launch_tcn_pw(td, gl + (2 * k + 1) * gper, W + tb.h[1].o_gamma, W + tb.h[1].o_beta,
                           W + tb.h[1].o_pw, cur, y, last ? bstride(n, L, B_D0) : 128LL * Tp, 0,
                           xs + (k + 1) * per, 128, T, Tp, N, s, (last && buf_oct(n, B_D0) == 3) ? n->bufs[B_D0].C : 0, tcn_x6));
      float* t = cur; cur = nxt; nxt = t;
    }
  }
  { int r = run_stack(n->dec); if (r) return r; }
  return MISONET_OK;
}

// ---------------------------------------------------------------------------------------------------------------
extern "C" {

const char* misonet_strerror(int code) {
  switch (code) {
    case MISONET_OK: return "ok";
    case MISONET_EINVAL: return "invalid argument / unsupported geometry";
    case MISONET_ESTATE: return "invalid call order or missing tensor";
    case MISONET_EHIP: return "HIP runtime error";
    case MISONET_ENOMEM: return "workspace too small";
    case MISONET_ENAN: return "NaN in network output";
    default: return "unknown error";
  }
}
const char* misonet_last_error(void) { return g_err; }
int misonet_version(void) { return 670; }   // 670: misonet_overiva_state_bytes, misonet_overiva_bins_per_pass, misonet_overiva_reset, misonet_overiva, misonet_overiva_debug (online AuxIVA for K < M sources; overiva.hip). 660: misonet_resample_stream_carry, misonet_resample_stream_state_bytes, misonet_resample_stream_outputs, misonet_resample_stream_tile, misonet_resample_stream_reset, misonet_resample_stream (streaming polyphase resampler: blocks in, blocks out, bits of misonet_resample); 650: misonet_stft_stream_state_bytes, misonet_stft_stream_reset, misonet_stft_stream_frames, misonet_stft_stream, misonet_istft_stream_state_bytes, misonet_istft_stream_reset, misonet_istft_stream_hops, misonet_istft_stream (streaming STFT / iSTFT: blocks in, blocks out, bits of the offline kernels); 640: misonet_obf_opts, misonet_obf_opts_default, misonet_obf_state_bytes, misonet_obf_cells_per_block, misonet_obf_reset, misonet_obf, misonet_obf_debug (online beamformer: frame-recursive MVDR / MWF, state carried); 630: misonet_oiva_opts, misonet_oiva_opts_default, misonet_oiva_state_bytes, misonet_oiva_bins_per_pass, misonet_oiva_reset, misonet_oiva, misonet_oiva_debug (online AuxIVA: frame-recursive separation, state carried); 620: misonet_owpe_opts, misonet_owpe_opts_default, misonet_owpe_state_bytes, misonet_owpe_lds_bytes, misonet_owpe_reset, misonet_owpe, misonet_owpe_debug (online WPE: frame-recursive, state carried); 610: misonet_doa_opts, misonet_doa_opts_default, misonet_doa_tile, misonet_doa_bin_chunk, misonet_doa_blocks, misonet_doa_workspace_bytes, misonet_doa, misonet_doa_debug (source localisation: SRP, SRP-PHAT and MUSIC maps); 600: misonet_room_tile, misonet_room_rir_len, misonet_room_mix_len, misonet_room_rir, misonet_room_mix (room simulator: image-source RIRs and scene mixing); 590: misonet_resample, misonet_resample_ratio, misonet_resampled_len, misonet_resample_taps, misonet_resample_tile (polyphase resampler for any rational rate); 580: misonet_iva_opts, misonet_auxiva, misonet_auxiva_debug, misonet_auxiva_workspace_bytes, misonet_auxiva_resident_frames (blind separation, AuxIVA-ISS); 570: misonet_jbf_opts, misonet_beamform_joint, misonet_beamform_joint_debug, misonet_pipeline_set_joint (joint multi-speaker beamformers); 560: misonet_cacgmm_opts, misonet_cacgmm, misonet_cacgmm_debug, misonet_masks_from_estimates, misonet_pipeline_set_refine (guided spatial clustering, cACGMM); 550: misonet_srmr_frames / misonet_srmr_scratch_bytes / misonet_srmr_chunk / misonet_srmr_measure (SRMR, the figure without a clean reference); 540: misonet_reverb_frames / misonet_reverb_scratch_bytes / misonet_reverb_measure (cepstral distance, LLR, fwSegSNR); 530: misonet_wpd_opts, misonet_wpd, misonet_wpd_debug, misonet_pipeline_set_wpd (WPD convolutional beamformer); 520: misonet_wpe_opts, misonet_wpe, misonet_wpe_debug (WPE dereverberation); 510: misonet_bf_opts, misonet_beamform, misonet_pipeline_set_beamformer (selectable beamformers: MPDR, Souden MVDR, GEV, BAN); 500: misonet_stoi_resample / misonet_stoi_measure (STOI and ESTOI); 490: misonet_bss_corr / misonet_bss_solve (BSS-eval SDR, SIR, SAR); 480: misonet_score_wave / misonet_score_spec (scores against clean references); 470: misonet_net_conv_plan (the kernel of every conv layer, decided at plan time); 460: misonet_css_align / misonet_css_stitch (continuous separation); 450:product modes 0 / 3 / 5 only (1, 2, 4, 6 answer MISONET_EINVAL); 410: misonet_pipeline_create accepts miso3 == NULL (separation-only pipeline); 420: misonet_istft; 430: misonet_frontend_init, precision mode 5 (f32w); 440: precision mode 6 (bf16x6w)

int misonet_net_create(const misonet_cfg* cfg, misonet_net** out) {
  if (!cfg || !out) return fail(MISONET_EINVAL, "null argument");
  misonet_net* n = new misonet_net();
  n->cfg = *cfg;
  int r = build_plan(n);
  if (r) { delete n; return r; }
  *out = n;
  return MISONET_OK;
}

int misonet_net_destroy(misonet_net* n) {
  if (!n) return MISONET_OK;
  if (n->w_dev) (void)hipFree(n->w_dev);
  delete n;
  return MISONET_OK;
}

int misonet_net_num_tensors(const misonet_net* n) { return n ? (int)n->tensors.size() : 0; }
const char* misonet_net_tensor_name(const misonet_net* n, int i) {
  if (!n || i < 0 || i >= (int)n->tensors.size()) return nullptr;
  return n->tensors[i].name.c_str();
}
long long misonet_net_tensor_numel(const misonet_net* n, int i) {
  if (!n || i < 0 || i >= (int)n->tensors.size()) return -1;
  return n->tensors[i].numel;
}

int misonet_net_set_tensor(misonet_net* n, const char* key, const float* host, long long numel) {
  if (!n || !key || !host) return fail(MISONET_EINVAL, "null argument");
  const int i = find_tensor(n, key);
  if (i < 0) return fail(MISONET_EINVAL, "unexpected state_dict key '%s'", key);
  if (n->tensors[i].numel != numel)
    return fail(MISONET_EINVAL, "size mismatch for '%s': expected %lld elements, got %lld", key, n->tensors[i].numel, numel);
  n->tensors[i].host.assign(host, host + numel);
  n->tensors[i].set = true;
  n->committed = false;
  return MISONET_OK;
}

// Run-time self-check of the f32w kernel, once per device at the first commit: conv3x3_wino_f32 drives 256 fixed
// AGPRs and hand-placed wait states through inline asm -- the build guard (tools/check_wino_build.py) covers what the compiler
// may do to it, this covers the machine: one small layer (40 -> 48 channels, 11 x 70, two samples: ragged row and column tiles, a
// 32-channel group on the 32-row body and 16 channels on the 16-row body) through the Winograd kernels AND through conv3x3_mfma,
// compared element by element.  A mismatch
// disables mode 5 on this device: misonet_net_set_precision(5) then fails loudly instead of computing garbage.
static std::atomic<int> g_wino_state[MAX_DEV] = {};          // 0 not checked, 1 ok, 2 failed
static std::mutex g_wino_mu;
static int wino_selftest() {
  const int d = cur_dev();
  int st = g_wino_state[d].load(std::memory_order_acquire);
  if (st) return st;
  std::lock_guard<std::mutex> lk(g_wino_mu);
  st = g_wino_state[d].load(std::memory_order_acquire);
  if (st) return st;
  const int Cin = 40, Cout = 48, F = 11, T = 70, Tp = frames_pitch(T), N = 2;   // (48 = a 32-channel group on the 32-row body + 16 channels on the 16-row body)
  std::vector<float> W((size_t)Cout * Cin * 9), bias(Cout), x((size_t)N * Cin * F * Tp);
  unsigned rng = 12345u;
  auto rnd = [&rng]() { rng = rng * 1664525u + 1013904223u; return (float)((int)(rng >> 9) - (1 << 22)) * (1.f / (1 << 22)); };
  for (float& v : W) v = 0.1f * rnd();
  for (float& v : bias) v = 0.3f * rnd();
  for (float& v : x) v = rnd();
  const ConvWeights cw = {W.data(), Cin, Cout, false, 64, 1};
  std::vector<float> wd((size_t)conv_image_floats(ConvKind::DIRECT, cw)), ww((size_t)conv_image_floats(ConvKind::WINO, cw));   // (ww: both bodies' images)
  conv_image_pack(ConvKind::DIRECT, cw, wd.data());
  conv_image_pack(ConvKind::WINO, cw, ww.data());
  const size_t out_n = (size_t)N * Cout * F * Tp, st_n = (size_t)N * Cout * 2 * DS_NL;
  float *dx = nullptr, *dwd = nullptr, *dww = nullptr, *db = nullptr, *dy = nullptr;
  dstat_t* dst = nullptr;
  auto release = [&]() { (void)hipFree(dx); (void)hipFree(dwd); (void)hipFree(dww); (void)hipFree(db); (void)hipFree(dy); (void)hipFree(dst); };
  bool ok = hipMalloc(reinterpret_cast<void**>(&dx), x.size() * 4) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&dwd), wd.size() * 4) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&dww), ww.size() * 4) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&db), 128 * 4) == hipSuccess &&
            hipMalloc(reinterpret_cast<void**>(&dy), 2 * out_n * 4) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&dst), 2 * st_n * 8) == hipSuccess;
  std::vector<float> y(2 * out_n);
  std::vector<dstat_t> sv(2 * st_n);
  if (ok) {
    std::vector<float> b128(128, 0.f);
    std::copy(bias.begin(), bias.end(), b128.begin());
    ok = hipMemcpy(dx, x.data(), x.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dwd, wd.data(), wd.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dww, ww.data(), ww.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(db, b128.data(), 128 * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemset(dy, 0, 2 * out_n * 4) == hipSuccess && hipMemset(dst, 0, 2 * st_n * 8) == hipSuccess;
  }
  if (ok) {
    ConvArgs a = {};
    a.in = dx; a.in_stats = nullptr; a.w = dwd; a.bias = db; a.ww = dww; a.ww16 = dww + conv_wino_ww16_at(Cin, Cout);
    a.in_bstride = (long long)Cin * F * Tp; a.out_bstride = (long long)Cout * F * Tp;
    a.in_sstride = Cin; a.out_sstride = Cout;
    a.in_c0 = 0; a.Cin = Cin; a.Fin = F; a.ident_c = Cin;              // input consumed as it is: no statistics to read
    a.out_c0 = 0; a.Cout = Cout; a.Fout = F; a.T = T; a.Tp = Tp;
    a.sf = 1; a.padf = 1; a.tr2 = 0; a.act = 1; a.ncg = 1; a.cop = 64;
    a.wscale = a.descale = 1.f;
    a.out = dy; a.out_stats = dst;
    ok = launch_conv_wino(a, N, nullptr) == hipSuccess;
    a.ww = nullptr; a.ww16 = nullptr; a.out = dy + out_n; a.out_stats = dst + st_n;
    ok = ok && launch_conv(a, N, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(y.data(), dy, 2 * out_n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(sv.data(), dst, 2 * st_n * 8, hipMemcpyDeviceToHost) == hipSuccess;
  }
  release();
  if (ok) {
    double worst = 0.0, scale = 0.0;
    for (int nn = 0; nn < N; ++nn)
      for (int c = 0; c < Cout; ++c)
        for (int f = 0; f < F; ++f)
          for (int t = 0; t < T; ++t) {
            const size_t i = (((size_t)nn * Cout + c) * F + f) * Tp + t;
            worst = std::max(worst, (double)fabsf(y[i] - y[out_n + i]));
            scale = std::max(scale, (double)fabsf(y[out_n + i]));
          }
    ok = std::isfinite(worst) && scale > 0.0 && worst <= 2e-5 * scale;
    for (size_t i = 0; ok && i < st_n / DS_NL; ++i) {                    // the statistics of both kernels (sum, sum of squares)
      auto rd = [](const dstat_t* p) { long long L[DS_NL]; for (int k = 0; k < DS_NL; ++k) L[k] = (long long)p[k]; return dstat_combine(L); };
      const double a1 = rd(sv.data() + i * DS_NL), a2 = rd(sv.data() + st_n + i * DS_NL);
      ok = std::isfinite(a1) && fabs(a1 - a2) <= 1e-4 * (fabs(a2) + 1.0);
    }
    if (!ok) fprintf(stderr, "[misonet] conv3x3_wino_f32 self-check FAILED on device %d (max |diff| %.3e of %.3e): mode f32w disabled\n", d, worst, scale);
  }
  st = ok ? 1 : 2;
  g_wino_state[d].store(st, std::memory_order_release);
  return st;
}

int misonet_net_commit(misonet_net* n) {
  if (!n) return fail(MISONET_EINVAL, "null argument");
  for (const Tensor& t : n->tensors)
    if (!t.set) return fail(MISONET_ESTATE, "missing state_dict key '%s'", t.name.c_str());
  long long off = 0;
  auto take = [&off](long long nfl) { long long o = off; off += (nfl + 63) / 64 * 64; return o; };
  // per conv layer: the bias, the direct image (always: the exact-f32 mode, the self-check's reference) and the image of every
  // other kind the plan holds for the layer over the three modes
  auto conv_weights = [n](const ConvL& c) { return ConvWeights{n->tensors[c.wt].host.data(), c.Cin, c.Cout, c.transposed, c.cop, c.ncg}; };
  for (std::vector<ConvL>* v : {&n->enc, &n->dec})
    for (ConvL& c : *v) {
      std::fill(c.img_off, c.img_off + CONV_NKIND, -1LL);
      c.img_off[(int)ConvKind::DIRECT] = take(conv_image_floats(ConvKind::DIRECT, conv_weights(c)));
      c.b_off = take((long long)c.ncg * c.cop);
      for (int mode = 0; mode < CONV_NMODES; ++mode) {
        long long& o = c.img_off[(int)c.kind[mode]];
        if (conv_mode_built(mode) && o < 0) o = take(conv_image_floats(c.kind[mode], conv_weights(c)));
      }
    }
  for (TcnBlock& tb : n->tcn)
    for (int h = 0; h < 2; ++h) {
      tb.h[h].o_dw = take(128 * 3);
      tb.h[h].o_prelu = take(1);
      tb.h[h].o_gamma = take(128);
      tb.h[h].o_beta = take(128);
      tb.h[h].o_pw = take(128 * 128);
      tb.h[h].o_nsc = take(128);
      tb.h[h].o_nsh = take(128);
    }
  std::vector<float> arena((size_t)off, 0.f);
  for (std::vector<ConvL>* v : {&n->enc, &n->dec})
    for (ConvL& c : *v) {
      for (int k = 0; k < CONV_NKIND; ++k)
        if (c.img_off[k] >= 0) conv_image_pack((ConvKind)k, conv_weights(c), arena.data() + c.img_off[k]);
      const std::vector<float>& Bv = n->tensors[c.bt].host;
      for (int co = 0; co < c.ncg * c.cop; ++co) arena[c.b_off + co] = co < c.Cout ? Bv[co] : 0.f;
    }
  for (const TcnBlock& tb : n->tcn)
    for (int h = 0; h < 2; ++h) {
      const TcnHalf& H = tb.h[h];
      memcpy(arena.data() + H.o_dw, n->tensors[H.dw].host.data(), 128 * 3 * sizeof(float));
      arena[H.o_prelu] = n->tensors[H.prelu].host[0];
      memcpy(arena.data() + H.o_gamma, n->tensors[H.gamma].host.data(), 128 * sizeof(float));
      memcpy(arena.data() + H.o_beta, n->tensors[H.beta].host.data(), 128 * sizeof(float));
      if (n->cfg.tcn_norm == 3) {                              // BatchNorm1d in eval mode (run.py:79,106): affine, eps 1e-5
        const float *w = n->tensors[H.on[0]].host.data(), *b = n->tensors[H.on[1]].host.data(),
                    *rm = n->tensors[H.on[2]].host.data(), *rv = n->tensors[H.on[3]].host.data();
        for (int ch = 0; ch < 128; ++ch) {
          const float sc = w[ch] / sqrtf(rv[ch] + 1e-5f);
          arena[H.o_nsc + ch] = sc;
          arena[H.o_nsh + ch] = b[ch] - rm[ch] * sc;
        }
      } else if (n->cfg.tcn_norm) {                            // gLN / cLN: gamma, beta
        memcpy(arena.data() + H.o_nsc, n->tensors[H.on[0]].host.data(), 128 * sizeof(float));
        memcpy(arena.data() + H.o_nsh, n->tensors[H.on[1]].host.data(), 128 * sizeof(float));
      }
      const std::vector<float>& P = n->tensors[H.pw].host;     // [co][ci][1] -> [ci][co]
      for (int co = 0; co < 128; ++co)
        for (int ci = 0; ci < 128; ++ci) arena[H.o_pw + (long long)ci * 128 + co] = P[(long long)co * 128 + ci];
    }
  if (n->w_dev) { (void)hipFree(n->w_dev); n->w_dev = nullptr; }
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&n->w_dev), arena.size() * sizeof(float)));
  HIPCHK(hipMemcpy(n->w_dev, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(conv_init());
  HIPCHK(conv_wino_init());
  HIPCHK(conv_few_init());
  if (wino_selftest() != 1 && n->precision == 5)
    return fail(MISONET_ESTATE, "the f32w kernel failed its self-check on this device (see stderr): use mode 0 (f32) or 3 (bf16x6)");
  HIPCHK(conv_bf16x6_init());
  { int rf = misonet_frontend_init(); if (rf) return rf; }     // STFT / iSTFT tables: never allocated inside an asynchronous call
  n->committed = true;
  return MISONET_OK;
}

int misonet_net_set_precision(misonet_net* n, int mode) {
  if (!n) return fail(MISONET_EINVAL, "null argument");
  if (mode < 0 || mode >= CONV_NMODES || !conv_mode_built(mode))
    return fail(MISONET_EINVAL, "precision mode must be 0 (f32), 3 (bf16x6) or 5 (f32w: f32 with the dense-block convs in Winograd form)");
  if (mode == 5 && g_wino_state[cur_dev()].load(std::memory_order_acquire) == 2)
    return fail(MISONET_ESTATE, "the f32w kernel failed its self-check on this device: mode 5 is disabled (use 0 or 3)");
  n->precision = mode;
  return MISONET_OK;
}
int misonet_net_get_precision(const misonet_net* n) { return n ? n->precision : -1; }

int misonet_net_buffer_plan(const misonet_net* n, int n_frames, int max_buffers, long long* offset_bytes,
                            long long* size_bytes, int* first_step, int* last_step) {
  if (!n || n_frames <= 0 || !offset_bytes || !size_bytes || !first_step || !last_step) return fail(MISONET_EINVAL, "null argument");
  const Layout L = make_layout(n, 1, n_frames);
  int k = 0;
  for (int b = 0; b < B_TXA && k < max_buffers; ++b, ++k) {
    offset_bytes[k] = L.data_off[b] * 4;
    size_bytes[k] = buf_floats(n, L.Tp, b) * 4;
    buf_lifetime(b, first_step[k], last_step[k]);
    if (n->keep_taps) { first_step[k] = 0; last_step[k] = 16; }
  }
  return k;
}

int misonet_net_conv_plan(const misonet_net* n, int mode, int max_layers, int* kind) {
  if (!n || !kind) return fail(MISONET_EINVAL, "null argument");
  if (mode < 0 || mode >= CONV_NMODES || !conv_mode_built(mode)) return fail(MISONET_EINVAL, "precision mode %d does not exist (0, 3, 5)", mode);
  int k = 0;
  for (const std::vector<ConvL>* v : {&n->enc, &n->dec})
    for (const ConvL& c : *v)
      if (k < max_layers) kind[k++] = (int)c.kind[mode];
  return k;
}

int misonet_net_keep_activations(misonet_net* n, int keep) {
  if (!n) return fail(MISONET_EINVAL, "null argument");
  n->keep_taps = keep != 0;
  return MISONET_OK;
}

long long misonet_net_workspace_bytes(const misonet_net* n, int n_samples, int n_frames) {
  if (!n || n_samples <= 0 || n_frames <= 0) return -1;
  return make_layout(n, n_samples, n_frames).total_bytes;
}

int misonet_net_forward(misonet_net* n, int n_seg, const void* const* seg_dev, const int* seg_ch, int B, int T,
                        void* out_dev, void* ws, long long ws_bytes, misonet_stream stream) {
  if (!n || !seg_dev || !seg_ch || !out_dev || !ws) return fail(MISONET_EINVAL, "null argument");
  if (!n->committed) return fail(MISONET_ESTATE, "misonet_net_commit has not been called");
  if (B <= 0 || T <= 0) return fail(MISONET_EINVAL, "B and T must be positive");
  int tot = 0;
  for (int i = 0; i < n_seg; ++i) tot += seg_ch[i];
  if (2 * tot != n->cfg.in_ch) return fail(MISONET_EINVAL, "input segments give %d complex channels, network expects %d", tot, n->cfg.in_ch / 2);
  const Layout L = make_layout(n, B, T);
  if (ws_bytes < L.total_bytes) return fail(MISONET_ENOMEM, "workspace %lld < %lld bytes", ws_bytes, L.total_bytes);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int c0 = 0;
  for (int i = 0; i < n_seg; ++i) {
    HIPCHK(launch_pack(reinterpret_cast<const float2*>(seg_dev[i]), B, seg_ch[i], T, n->cfg.n_freq, buf_ptr(L, ws, B_IN),
                       bstride(n, L, B_IN), L.Tp, c0, tot + c0, 1, s));
    c0 += seg_ch[i];
  }
  int r = forward_planar(n, L, ws, s);
  if (r) return r;
  HIPCHK(launch_unpack(buf_ptr(L, ws, B_OUT), bstride(n, L, B_OUT), L.Tp, n->S, T, n->cfg.n_freq,
                       reinterpret_cast<float2*>(out_dev), B, reinterpret_cast<int*>(ws), s));
  return MISONET_OK;
}

int misonet_net_check(misonet_net* n, const void* ws, misonet_stream stream) {
  if (!n || !ws) return fail(MISONET_EINVAL, "null argument");
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, ws, sizeof(int), hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(stream)));
  HIPCHK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  if (flag) return fail(MISONET_ENAN, "NaN in network output");
  return MISONET_OK;
}

int misonet_net_tap_shape(const misonet_net* n, const char* name, int* C, int* F) {
  if (!n || !name) return fail(MISONET_EINVAL, "null argument");
  for (const Tap& t : n->taps)
    if (t.name == name) {
      if (C) *C = t.C;
      if (F) *F = n->bufs[t.buf].F;
      return MISONET_OK;
    }
  return fail(MISONET_EINVAL, "unknown tap '%s'", name);
}

int misonet_net_tap(misonet_net* n, const char* name, const void* ws, int B, int T, float* dst, misonet_stream stream) {
  if (!n || !name || !ws || !dst) return fail(MISONET_EINVAL, "null argument");
  const Layout L = make_layout(n, B, T);
  for (const Tap& t : n->taps)
    if (t.name == name) {
      if (!n->keep_taps && t.buf != B_OUT)
        return fail(MISONET_ESTATE, "tap '%s': activation buffers share memory; call misonet_net_keep_activations(net, 1) "
                                    "before the forward", name);
      {
        // the plan the workspace was WRITTEN with must be the one this call would read it with (a diagnostic entry point:
        // the 4-byte read-back synchronises the stream)
        unsigned stamp = 0;
        hipStream_t s_ = reinterpret_cast<hipStream_t>(stream);
        HIPCHK(hipMemcpyAsync(&stamp, reinterpret_cast<const char*>(ws) + 8, sizeof(stamp), hipMemcpyDeviceToHost, s_));
        HIPCHK(hipStreamSynchronize(s_));
        if (stamp != layout_stamp(n, L))
          return fail(MISONET_ESTATE, "tap '%s': the forward in this workspace ran with another buffer plan / mode / shape "
                                      "(keep_activations, precision, B or T changed since); run the forward again", name);
      }
      void* w = const_cast<void*>(ws);
      HIPCHK(launch_export(buf_ptr(L, w, t.buf), bstride(n, L, t.buf), t.c0, t.C, n->bufs[t.buf].F, T, L.Tp,
                           t.normalised ? stats_ptr(L, w, t.buf) : nullptr, n->bufs[t.buf].C, 0, dst, B,
                           reinterpret_cast<hipStream_t>(stream), buf_oct(n, t.buf) >= 3 ? buf_oct(n, t.buf) : (buf_oct(n, t.buf) ? 2 : 0)));
      return MISONET_OK;
    }
  return fail(MISONET_EINVAL, "unknown tap '%s'", name);
}

// ---- per-launch profiling -----------------------------------------------------------------------------------------
int misonet_profile_begin(int max_launches) {
  if (max_launches <= 0) return fail(MISONET_EINVAL, "max_launches must be positive");
  Prof& pr = g_profs[cur_dev()];
  while (pr.pool.size() < (size_t)max_launches * 2) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    pr.pool.push_back(e);
  }
  pr.used = 0;
  pr.recs.clear();
  pr.overflow = false;
  if (!pr.on) g_prof_any.fetch_add(1);
  pr.on = true;
  return MISONET_OK;
}
int misonet_profile_end(double* ms_by_kind, long long* launches_by_kind) {
  Prof& pr = g_profs[cur_dev()];
  if (pr.on) g_prof_any.fetch_sub(1);
  pr.on = false;
  if (!ms_by_kind || !launches_by_kind) return fail(MISONET_EINVAL, "null argument");
  for (int k = 0; k < PK_N; ++k) { ms_by_kind[k] = 0.0; launches_by_kind[k] = 0; }
  for (const ProfRec& r : pr.recs) {
    HIPCHK(hipEventSynchronize(r.e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
    ms_by_kind[r.kind] += ms;
    launches_by_kind[r.kind] += 1;
  }
  if (pr.overflow) return fail(MISONET_ENOMEM, "profile event pool exhausted");
  return MISONET_OK;
}

// ---- events --------------------------------------------------------------------------------------------------------
int misonet_event_create(void** ev) {
  hipEvent_t e;
  HIPCHK(hipEventCreate(&e));
  *ev = e;
  return MISONET_OK;
}
int misonet_event_record(void* ev, misonet_stream stream) {
  HIPCHK(hipEventRecord(reinterpret_cast<hipEvent_t>(ev), reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}
int misonet_event_elapsed_ms(void* start, void* stop, float* ms) {
  HIPCHK(hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop)));
  HIPCHK(hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(start), reinterpret_cast<hipEvent_t>(stop)));
  return MISONET_OK;
}
int misonet_event_destroy(void* ev) {
  HIPCHK(hipEventDestroy(reinterpret_cast<hipEvent_t>(ev)));
  return MISONET_OK;
}

}  // extern "C"
