// Internal declarations shared by the HIP translation units of libmisonet_hip.so (gfx950 only).
//
// Activation layout in HBM ("planar"): float32 [n][c][f][Tp], frames (t) innermost, Tp = T rounded up to 32 so
// every row starts 128-byte aligned.  Conv outputs are stored RAW (bias + ELU applied, instance norm NOT applied);
// each producer accumulates per-(n,c) sum / sum-of-squares exactly (det_stats.hpp) next to the buffer and every consumer
// normalises while it stages its input tile into LDS ("normalise on load").  Dense-block concatenation is free:
// a block's tensors are channel slices of one buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "det_stats.hpp"
#include "sig_view.hpp"

namespace mn {

constexpr int CK = 8;       // input channels per K-chunk of the implicit GEMM
constexpr int TT = 128;     // output frames per workgroup (4 MFMA column tiles of 32)
constexpr int TW = 136;     // staged frames per input row: [t0-4, t0+132) -> 34 aligned float4
constexpr int FT = 4;       // output rows (frequency bins) per workgroup = waves per workgroup
constexpr float IN_EPS = 1e-5f;    // nn.InstanceNorm{1,2}d default eps (reference model.py:413,579)
constexpr float GLN_EPS = 1e-8f;   // reference model.py:6

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
inline int frames_pitch(int T) { return round_up(T, 32); }

// ---- 3x3 convolution family (reference model.py:401-482), one launch per layer ------------------------------
struct ConvArgs {
  const float* in;          // planar buffer base
  const dstat_t* in_stats;  // [n][in_sstride][2][DS_NL] (sum, sumsq as det_stats.hpp limbs) or nullptr when every input channel is identity
  float* out;
  dstat_t* out_stats;       // [n][out_sstride][2][DS_NL], accumulated with integer atomics (ds_add) when act != 0
  const float* w;           // packed [ncg][nchunk][9][CK][COP]
  const float* bias;        // [ncg*COP]
  // Fields marked (constant) hold the same value in every launch since the measured alternative modes (bf16x3, f16x3, bf16x6w) and
  // the timing switches left the library.  They remain because the struct's byte layout, and with it every kernel's argument
  // offsets and code, stays what it was; the device-side tests of `dbg` are listed in LAB.md ("Leftovers of the experiment build").
  const unsigned short* w16; // (constant) nullptr
  const void* ww6;          // (constant) nullptr
  const float* wsm;         // conv_few.hip (<= 4 output channels): [Cin][9 = kt * 3 + kf][4 co] conv-form taps, or nullptr
  const float* ww16;        // f32w path: the LAST 16 output channels of a layer with Cout % 32 == 16 as their own Winograd image for the 16-row body
                            // (conv_wino.hip G16): [chunk of 8][K-step of 4 ci][pos / 4][ci % 4][16 co][pos % 4], or nullptr
  const float* w1d;         // f32w path, frequency-strided layers (conv.hip W1D): 1-D Winograd weights along T, [cg32][chunk of 8][nu * 3 + kf][ci][32 co], or nullptr
  const float* ww;          // f32w path (conv_wino.hip): Winograd-domain weights U = G g G^T, [cg32][chunk of 8][pos / 4][ci][32 co][pos % 4], or nullptr
  long long in_bstride;     // floats per sample of the input buffer
  long long out_bstride;
  int in_sstride, out_sstride;   // channels per sample in the stats arrays (= channels of the whole buffer)
  int in_c0, Cin, Fin;
  int ident_c;              // input channels [0, ident_c) are consumed as they are (no instance norm)
  int out_c0, Cout, Fout;
  int T, Tp;
  int sf;                   // frequency stride of a forward conv (1 or 2)
  int padf;                 // frequency zero padding of the conv form (0, 1, or 2 for a stride-1 transposed conv)
  int tr2;                  // 1: stride-2 transposed conv (fin = (f + kf - 2) / 2 when even)
  int act;                  // 1: ELU + statistics for the following instance norm; 0: raw output
  int NR;                   // staged input rows per workgroup (set by the launcher)
  int ncg;                  // output-channel groups (grid.z = n_samples * ncg)
  int cop;                  // 32 or 64 output channels per group
  int in_oct, out_oct;      // layout of the input / output buffer: 0 planar float32, 3 oct3 (bf16x6, conv_bf16x6.hip: per sample
                            // [hi | mid | lo] parts, each [c/8][f][Tp][8] bf16, 6 bytes per element; values RAW: bias + ELU, no norm)
  float wscale, descale;    // (constant) 1, 1
  const void* wps;          // per-sample weights with the instance norm of the input folded in (conv_wprep), LDS image order
  long long wps_nstride;    // bytes between samples (0: one image shared by all samples)
  const float* btab;        // [n][ncg*32][9] border-aware shift table: sum_ci W[co][ci][tap] * shift[ci], or nullptr
  long long btab_nstride;   // floats between samples
  int xcd;                  // 1: 1-D grid with the XCD-aware tile order of conv_tile() (ntx, nty, nsamp valid)
  int ntx, nty, nsamp;      // frame tiles, row tiles, samples of this launch
  unsigned long long* dbg_buf;   // (constant) nullptr: where the timeline experiments had one workgroup write its clock stamps
  int dbg;                  // (constant) 0: ablation bits of the timing experiments (1 skip MFMAs, 4 skip epilogue, 8 skip stores,
                            // 16 skip statistics reductions, 32 no deferred epilogue)
};
// Workgroup -> tile.  Hardware hands consecutive workgroup ids to the 8 XCDs round-robin and every XCD has its own
// L2, so with the natural (t, f, n) order the 8 frame tiles of a row sit on 8 different XCDs and every halo line is
// fetched twice.  XCD order: id & 7 picks the XCD, id >> 3 walks that XCD's own samples (n % 8 == xcd) tile by
// tile (frame tile fastest, then output-channel group, then row tile): all tiles that share halos or re-read the same
// input with another channel group are co-resident on ONE XCD.
struct ConvTile { int t_tile, f_tile, n, cg; bool valid; };
__device__ __forceinline__ ConvTile conv_tile(const ConvArgs& a) {
  ConvTile r;
  if (a.xcd) {
    const unsigned id = blockIdx.x;
    const unsigned xcd = id & 7u, k = id >> 3;
    const unsigned per = (unsigned)(a.ntx * a.nty * a.ncg);
    const unsigned grp = k / per;
    unsigned tile = k - grp * per;
    r.n = (int)(grp * 8u + xcd);
    r.t_tile = (int)(tile % (unsigned)a.ntx);
    tile /= (unsigned)a.ntx;
    r.cg = (int)(tile % (unsigned)a.ncg);
    r.f_tile = (int)(tile / (unsigned)a.ncg);
    r.valid = r.n < a.nsamp;
  } else {
    r.t_tile = blockIdx.x; r.f_tile = blockIdx.y;
    r.n = blockIdx.z / a.ncg; r.cg = blockIdx.z - r.n * a.ncg;
    r.valid = true;
  }
  return r;
}
// fills xcd/ntx/nty/nsamp and returns the launch grid
inline dim3 conv_grid(ConvArgs& a, int n_samples, int tt, int ft, int xcd) {
  a.ntx = (a.T + tt - 1) / tt; a.nty = (a.Fout + ft - 1) / ft; a.nsamp = n_samples; a.xcd = xcd;
  if (xcd) return dim3((unsigned)(8 * ((n_samples + 7) / 8) * a.ntx * a.nty * a.ncg), 1, 1);
  return dim3(a.ntx, a.nty, n_samples * a.ncg);
}
int device_cus();                            // compute units of the CURRENT device (cached per device, thread-safe); <= 0 on error
int conv_cop(int Cout);                      // 32 (Cout <= 32) or 64
// Which of these launchers runs a layer: conv_select.hpp (one ConvKind per layer and arithmetic mode, with the launchers' own guards).
// Every launcher answers hipErrorInvalidValue to a layer its kernel does not take, and sets ConvArgs::NR itself.
hipError_t launch_conv(const ConvArgs& a, int n_samples, hipStream_t s);       // any shape (needs a.w)
// f32w, the frequency-strided layers and the first layer in 1-D Winograd form along T (conv.hip W1D; needs a.w1d)
hipError_t launch_conv_w1d(const ConvArgs& a, int n_samples, hipStream_t s);
hipError_t conv_init();                      // dynamic-LDS attributes
// Winograd F(2x2, 3x3) on the fp32 matrix cores for the stride-1 same-padded layers (conv_wino.hip; precision mode "f32w"; needs a.ww)
hipError_t launch_conv_wino(const ConvArgs& a, int n_samples, hipStream_t s);
hipError_t conv_wino_init();
// <= 4 output channels, stride 1, no activation (the network's last layer) on the vector ALU (conv_few.hip; needs a.wsm)
hipError_t launch_conv_few(const ConvArgs& a, int n_samples, hipStream_t s);
hipError_t conv_few_init();
// bf16x6 (fp32-faithful) DMA dataflow, conv_bf16x6.hip: oct3 input, oct3 or planar output
hipError_t launch_conv_bf16x6(const ConvArgs& a, int n_samples, hipStream_t s);
hipError_t launch_conv_wprep6(const ConvArgs& a, const float* wf6, int n_samples, hipStream_t s);
hipError_t conv_bf16x6_init();
long long conv_bf16x6_wps_bytes(int Cin, int Cout);   // per-sample folded-weight bytes of one layer
// the network's first layer in the bf16x6 arithmetic: planar float32 in (consumed as it is), oct3 / planar out; wimg = the
// layer's weights as ONE 3-part image per 8-channel chunk (864 16-byte units each, conv_wprep6_k's order; net.hip packs it)
hipError_t launch_conv_x6_first(const ConvArgs& a, const void* wimg, int n_samples, hipStream_t s);

// ---- TCN (reference model.py:486-632) -----------------------------------------------------------------------------
// Statistics travel as float64 (sum, sum of squares) PARTIALS, one per producing workgroup, added by the consumer in index
// order (no atomics, bit-reproducible): IN1d [n][C][tcn_part_slots(T)] (one per 128-frame tile; tcn_prepare writes slot 0
// only), gLN [n][C / 4] (one per 4-channel group).
int tcn_part_slots(int T);
// x0 = IN2d(raw) materialised as the residual stream + its per-(n,c) statistics
hipError_t launch_tcn_prepare(const float* raw, long long raw_bstride, int raw_c0, const dstat_t* raw_stats, int raw_sstride,
                              float* x, double2* x_part, int C, int T, int Tp, int n_samples, hipStream_t s,
                              int raw_oct3 = 0);   // raw_oct3: source in the bf16x6 oct3 layout
// d = PReLU(dwconv_dilated(ELU(norm(x)))) ; gLN partials of d.  x_np: partials per row of x_part (1 or tcn_part_slots(T)).
// norm = the TemporalBlock's outer norm (model.py:530,535; chose_norm model.py:570-581), norm_kind: 0 InstanceNorm1d;
// 1 gLN over (C, T) of a sample with (nsc, nsh) = (gamma, beta) per channel; 2 cLN over the channels of every frame with
// (gamma, beta) and fstat [n][Tp] (mean, rstd) from launch_tcn_cln_stats; 3 BatchNorm1d in eval mode with (nsc, nsh) = the
// folded (weight / sqrt(running_var + eps), bias - running_mean * that) per channel.
hipError_t launch_tcn_dw(const float* x, const double2* x_part, int x_np, const float* wdw /*[C][3]*/, const float* prelu /*[1]*/,
                         float* d, double2* gln_part /*[n][C/4]*/, int C, int T, int Tp, int dilation, int n_samples, hipStream_t s,
                         int norm_kind = 0, const float* nsc = nullptr, const float* nsh = nullptr, const float2* fstat = nullptr);
// per-frame mean / rstd over the C channels of x [n][C][Tp] (ChannelwiseLayerNorm, model.py:583-606): fstat [n][Tp]
hipError_t launch_tcn_cln_stats(const float* x, float2* fstat, int C, int T, int Tp, int n_samples, hipStream_t s);
// y = pwconv(gLN(d)) (+ residual) ; IN partials of y
hipError_t launch_tcn_pw(const float* d, const double2* gln_part, const float* gamma, const float* beta,
                         const float* wpw /*packed [C/CK... see tcn.hip]*/, const float* residual /*or nullptr*/,
                         float* y, long long y_bstride, int y_c0, double2* y_part /*[n][C][slots]*/, int C, int T, int Tp,
                         int n_samples, hipStream_t s,
                         int y_oct3_cbuf = 0, int x6 = 0);   // != 0: y is an oct3 buffer with that many channels (bf16x6 mode)

// ---- layout conversion ----------------------------------------------------------------------------------------
// complex64 [B][Mseg][T][F] -> planar real/imag channel planes; optional circular mic shifts (tester.py:1034,1050):
// destination sample n = b*nshift + k receives source channel (m + k) % Mseg at destination channel m.
hipError_t launch_pack(const float2* src, int B, int Mseg, int T, int F, float* dst, long long dst_bstride, int Tp,
                       int c_re, int c_im, int nshift, hipStream_t s);
// planar [n][2S][F][Tp] -> complex64 [n][S][T][F]; sets *nan_flag when a NaN is seen (model.py:109-110)
hipError_t launch_unpack(const float* src, long long src_bstride, int Tp, int S, int T, int F, float2* dst, int n_samples,
                         int* nan_flag, hipStream_t s);
// planar view (+ optional instance norm) -> float32 [n][C][T][F]  (diagnostic taps)
hipError_t launch_export(const float* src, long long src_bstride, int c0, int C, int Fq, int T, int Tp,
                         const dstat_t* stats, int sstride, int ident_c, float* dst, int n_samples, hipStream_t s,
                         int oct = 0);   // oct: 0 planar, 3 a source in the oct3 layout (sstride = channels of the
                                         // whole buffer)
// what the fused pipeline adds: launch_unpack's general form (layout.hip: real / imaginary planes from channel c_re0 / c_im0 on,
// sources picked through sel); the shift and clean alignments composed into one sel, and the MISO3 input [mixture | beamformer
// planes, written by launch_mvdr | MISO1 estimate at ref_ch] (both mvdr.hip)
hipError_t launch_unpack_ex(const float* src, long long src_bstride, int Tp, int S, int T, int F, int c_re0, int c_im0, int mode,
                            int M, const int* sel, float2* dst, int n_out, int* nan_flag, hipStream_t s);
hipError_t launch_compose_sel(const int* shift_sel, const int* clean_sel, int B, int M, int S, int* out, hipStream_t s);
hipError_t launch_assemble3(const float* in1, long long in1_bstride, const float* out1, long long out1_bstride,
                            const int* sel, int B, int M, int S, int ref_ch, int F, int Tp, float* in3,
                            long long in3_bstride, hipStream_t s);

// ---- STFT front-end (stft.hip) --------------------------------------------------------------------------------------
// waveform -> planar network input, and complex64 spectrum -> waveform; each reads a twiddle table built on the host
// (*_twiddle_count() floats) and needs its *_init() once per device (kernel attributes)
hipError_t launch_stft_pack(const float* wav, int B, int L, int Mw, int T, const float* twid, float* dst,
                            long long dst_bstride, int Tp, int F, int c_re, int c_im, int nshift, hipStream_t s);
hipError_t stft_init();
void stft_build_twiddles(float* tw);
int stft_twiddle_count();
hipError_t launch_istft(const void* spec, int N, int T, const float* itw, short* out_i16, float* out_f32, hipStream_t s);
hipError_t istft_init();
void istft_build_twiddles(float* tw);
int istft_twiddle_count();
// The streaming forms: the same tables, and stft_stream_init() once per device.  The state of the analysis
// is float [B M][256] (the last 255 samples, then one zero), that of the synthesis complex64 [R][3][129] (the last 3 frames);
// zero bytes are the reset.  launch_stft_stream: Tn frames, the first starting off0 in [-255, 0] samples from the block's first
// sample (nothing is launched for Tn == 0), then, with `update`, the tail after the block's n samples.  launch_istft_stream: H
// hops, hop 0 of the call summing the frames fr0 .. fr0 + 3 counted from the first new frame, of which the `lead` <= 3 last
// carried ones and the Tn new ones exist; then, with `update`, the carried frames after the Tn >= 1 new ones.
long long stft_stream_state_bytes(long long BM);
long long istft_stream_state_bytes(long long R);
hipError_t stft_stream_init();
hipError_t launch_stft_stream(const float* wav, int B, int n, int Mw, int Tn, int off0, int update, const float* twid,
                              float2* out, float* tail, hipStream_t s);
hipError_t launch_istft_stream(const void* spec, int R, int Tn, int lead, int fr0, int H, int update, const float* itw,
                               short* out_i16, float* out_f32, void* carry, hipStream_t s);

// ---- MVDR + PIT -------------------------------------------------------------------------------------------------
// Accessor for a multichannel complex STFT with frames contiguous: element (b, f, m, t) =
//   re[b*sb + f*sf + m*sm + t*st], im likewise.  Interleaved complex64 [B,F,M,T]: re=base, im=base+1, st=2.
struct CView {
  const float* re; const float* im;
  long long sb, sf, sm; int st;
};
enum { BF_MVDR = 0, BF_SOUDEN = 1, BF_GEV = 2 };
struct MvdrArgs {
  CView mix;             // observation Y
  const float* est;       // planar MISO1 output buffer [B*M][2S][F][Tp] (pipeline mode) or nullptr
  long long est_bstride;  // floats per sample
  const int* sel;         // [B][M][S]: estimated-speaker index to use for (b, mic m, aligned speaker j), or nullptr
  CView src;              // source estimate S when est == nullptr (drop-in mode)
  int S;                  // speakers handled per utterance (grid.z)
  int B, F, M, T, Tp;
  float epsi;
  // the beamformer (misonet_bf_opts, already validated on the host); the defaults are the reference's live path
  int kind = BF_MVDR;     // BF_MVDR / BF_SOUDEN / BF_GEV
  int noise_mix = 0;      // 1: Phi_n from Y instead of Y - S (MPDR, tester.py:1096)
  int trace_norm = 0;     // Phi_n <- Phi_n / tr(Phi_n) (tester.py:1099)
  int ban = 0;            // blind analytic normalisation of w (tester.py:1186-1208)
  int bf_ref = 0;         // reference microphone of souden / gev
  double condition = 0.0; // gamma: Phi_n <- (Phi_n + gamma tr(Phi_n) / M I) / (1 + gamma), per bin
};
long long mvdr_ws_bytes(int B, int S, int F, int M);
// workspace of launch_mvdr for a kind: mvdr_ws_bytes, for souden / gev followed by Phi_s [B][S][F][M][M] and lambda_max [B][S][F]
long long bf_ws_bytes(int B, int S, int F, int M, int kind);
// out: complex, element (b, spk, t, f) at out_re[b*ob + spk*os + t*ot + f*of]
struct COut { float* re; float* im; long long ob, os, ot, of; };
hipError_t launch_mvdr(const MvdrArgs& a, const COut& out, void* ws, hipStream_t s);
hipError_t launch_mvdr_debug(const void* ws, int B, int S, int F, int M, double* steer, double* w, hipStream_t s);
// w complex128 [B][S][F][M] and (gev only) lambda_max float64 [B][S][F] of the last launch_mvdr in ws; either may be null
hipError_t launch_bf_debug(const void* ws, int B, int S, int F, int M, double* w, double* lam, hipStream_t s);

// dist[b][i][j] = sum_{t,f} | |A_i| - |B_j| | for S = 1..4 speakers: per-bin float64 partials, added in bin order (bit-
// reproducible); then sel = the cheapest of the S! permutations (itertools order, first minimum).
struct PitArgs {
  CView a, b;             // sm = speaker stride here; (b, f, spk, t) addressing
  int B, F, T;
};
// K candidates per anchor: grid row bk = b*K + k uses anchor b and candidate bk
hipError_t launch_pit_dist_k(const PitArgs& p, int S, int K, double* part /*[B*K][F][S][S]*/, hipStream_t s);
hipError_t launch_pit_pick(const double* part, int F, int S, int n, double* dist /*[n][S][S]*/, int* sel /*[n][S]*/, hipStream_t s);

// Continuous separation (css.hip): the window-to-window permutations composed along the recording, and the cross-fade stitch
hipError_t launch_css_chain(const int* perm0, int* perm, int K, int S, hipStream_t s);
hipError_t launch_css_stitch(const float* y, const int* perm, int K, int S, int W, int hop, long long base, long long n_out,
                             short* out_i16, float* out_f32, hipStream_t s);

// Scores of separated output against clean references (score.hip).  Wave statistics over the estimates and the references
// (SigView, sig_view.hpp): per-segment partials [B][score_wave_segments(n)][2E + 2R + E R] are folded in segment order into
// stats [B][E][R][5] = (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j), an int16 estimate scaled by 1 / 32767 once.
// 1 <= E <= 5, 1 <= R <= 4.
long long score_wave_segments(long long n);
hipError_t launch_score_wave(const SigView& est, const SigView& ref, int B, int E, int R, long long n,
                             const int* n_valid /*[B] or nullptr*/, double* part, double* stats, hipStream_t s);
// The spectral training criterion per pair: p.a = estimates, p.b = references, sm = the source stride; per-bin partials
// [B][F][E][R] folded in bin order into pair [B][E][R]; perm [B][R] / upit [B] (either may be nullptr; E == R): the uPIT pick
hipError_t launch_score_spec(const PitArgs& p, int E, int R, double* part, double* pair, int* perm, double* upit,
                             hipStream_t s);

// BSS-eval energies (bss.hip).  Lagged correlations over the same views as launch_score_wave: per-segment partials
// [B][bss_corr_segments(n)][R R + R E + E][Q] folded in segment order into Rrr [B][R][R][Q], Rre [B][R][E][Q], Eee [B][E].
// The systems: per item bss_solve_doubles(R, Q) doubles of scratch; T [B][E][R], A [B][E], info [B] (-1, or the first row
// whose pivot failed).  1 <= E, R <= 4, 16 | Q, 16 <= Q <= 1024.
long long bss_corr_segments(long long n);
long long bss_solve_doubles(int R, int Q);
hipError_t launch_bss_corr(const SigView& est, const SigView& ref, int B, int E, int R, long long n,
                           const int* n_valid /*[B] or nullptr*/, int Q, double* part, double* Rrr, double* Rre, double* Eee,
                           hipStream_t s);
hipError_t launch_bss_solve(const double* Rrr, const double* Rre, int B, int E, int R, int Q, double* T, double* A, int* info,
                            double* scratch, hipStream_t s);

// STOI / ESTOI (stoi.hip).  The table (stoi_table_count() doubles, built on the host): the window, the
// twiddles of the 512-point transform and the polyphase taps of 16, 8 and 10 kHz.  The resampler reads the three views (the
// mixture's p may be nullptr) and writes x10 [B][R + E (+ 1)][n10] (references, estimates, mixture) and len10 [B].  The measure: per item stoi_item_doubles(NS, R, n10) doubles of scratch;
// out [B][NS - R][R][2] = (STOI, ESTOI), meta [B][R][3] = (frames, kept frames, any sample != 0).
int stoi_table_count();
void stoi_build_table(double* t);
int stoi_taps(int fs);            // 2 Lh + 1, or -1 for a rate that is not served
int stoi_tap_offset(int fs);      // where those taps start in the table, or -1
long long stoi_resampled_len(long long n, int fs);
long long stoi_item_doubles(int NS, int R, long long n10);
hipError_t launch_stoi_resample(const SigView& est, const SigView& ref, const SigView& mix, int B, int E, int R, long long n,
                                const int* n_valid /*[B] or nullptr*/, int fs, const double* table, double* x10, int* len10,
                                hipStream_t s);
hipError_t launch_stoi_measure(const double* x10, const int* len10 /*[B] or nullptr*/, int B, int NS, int R, long long n10,
                               const double* table, double* out, int* meta, double* scratch, hipStream_t s);

// Polyphase resampler for any rational rate (resample.hip): scipy.signal.resample_poly's definition, p / q =
// fs_out / fs_in in lowest terms with max(p, q) <= RS_MAX_RATE.  The taps g[0 .. 2 Lh] of one (p, q) are built on the host
// (resample_build_taps) and kept on the device by the caller.  src float32 or int16, element (b, c, j) at b ss[0] + c ss[1] +
// j ss[2]; dst float32 or int16 likewise through ds; y[m] = sum_j x[j] g[m q - j p + Lh], j ascending, in float64, rounded once;
// outputs past ceil(n_valid[b] p / q) are zeros.  1 <= M <= RS_MAX_CH, 1 <= B <= 65535: the caller checks them.
constexpr int RS_MAX_RATE = 1024;
constexpr int RS_MAX_CH = 16;
bool resample_ratio(long long fs_in, long long fs_out, int* p, int* q);   // false: a rate < 1 or max(p, q) > RS_MAX_RATE
int resample_half_len(int p, int q);                                      // Lh: 10 max(p, q), 0 for 1 / 1
long long resample_len(long long n, int p, int q);                        // ceil(n p / q)
void resample_build_taps(int p, int q, double* g /*[2 Lh + 1]*/);
int resample_tile();                                                      // output samples per workgroup
hipError_t launch_resample(const void* src, int src_i16, const long long* ss, int B, int M, long long n,
                           const int* n_valid /*[B] or nullptr*/, int p, int q, const double* taps, void* dst, int dst_i16,
                           const long long* ds, hipStream_t s);

// The streaming form (resample_stream.hip): the same taps.  After N samples a stream has emitted
// resample_stream_emitted(N) outputs and carries its last resample_stream_carry(p, q) samples, float32 [B][M][C] aligned to its
// end, zero where it has not begun.  launch_resample_stream: the n_out outputs from e(N) on (nothing is launched for n_out == 0),
// D = e(N) q - N p, then, with `update`, the tail after the block's n_new samples.  N itself is no argument.
int resample_stream_tile();                                               // output samples per workgroup
int resample_stream_carry(int p, int q);                                  // C = floor(2 Lh / p)
long long resample_stream_emitted(long long N, int p, int q);             // e(N)
hipError_t launch_resample_stream(const void* src, int src_i16, const long long* ss, int B, int M, long long n_new, long long D,
                                  long long n_out, int update, int p, int q, const double* taps, void* dst, int dst_i16,
                                  const long long* ds, float* tail /*nullptr where C == 0*/, hipStream_t s);

// Cepstral distance, LLR and fwSegSNR (reverb.hip).  The table (reverb_table_count() doubles, built on the
// host): the twiddles of the 512-point transform and, per rate, the window, the 23 mel triangles and their bin ranges.  One call
// reads the three views of launch_stoi_resample and writes out [B][E (+ 1)][R][6], count
// [B][E (+ 1)][R][3] and, where frame_out is not nullptr, the values of every frame [B][E (+ 1)][R][3][frames of n]; per item
// reverb_item_doubles(NS, R, n, fs) doubles of scratch, NS = R + E (+ 1).
int reverb_table_count();
void reverb_build_table(double* t);
long long reverb_frames(long long n, int fs);      // -1 for a rate that is not served or n outside 1 .. 2^24
long long reverb_item_doubles(int NS, int R, long long n, int fs);
hipError_t launch_reverb_measure(const SigView& est, const SigView& ref, const SigView& mix, int B, int E, int R, long long n,
                                 const int* n_valid /*[B] or nullptr*/, int fs, const double* table, double* out, int* count,
                                 double* frame_out /*or nullptr*/, double* scratch, hipStream_t s);

// SRMR, the speech-to-reverberation modulation energy ratio (srmr.hip).  The table (srmr_table_count() doubles,
// built on the host): the twiddles of the transforms and, per rate, the window, the gammatone and modulation coefficients, their
// chunk-to-chunk transitions A^C, ERB(cf_j) and the lower cutoffs ll_k.  One call reads the S signals of sig and, where mix.p is
// not nullptr, the mixture as one more signal, the last, and writes out [B][S (+ 1)][3] = (SRMR, K*, BW), count [B][S (+ 1)] =
// the frames and, where energy is not nullptr, the mean modulation energies [B][S (+ 1)][23][8];
// srmr_scratch_doubles(B, S (+ 1), n, fs) doubles of scratch.
int srmr_table_count();
void srmr_build_table(double* t);
int srmr_chunk();                                  // C of the chunked scan
long long srmr_frames(long long n, int fs);        // -1 for a rate that is not served or n outside 0 .. 2^24
long long srmr_scratch_doubles(int B, int NS, long long n, int fs);   // -1 outside the limits
hipError_t launch_srmr_measure(const SigView& sig, const SigView& mix, int B, int S, long long n,
                               const int* n_valid /*[B] or nullptr*/, int fs, const double* table, double* out, int* count,
                               double* energy /*or nullptr*/, double* scratch, hipStream_t s);

// WPE dereverberation (wpe.hip).  mix / out complex64 [B][M][T][F], power float32 [B][T][F] or nullptr; the
// workspace starts with fail int [B F] and G complex128 [B F][M taps][M], which launch_wpe_debug copies out.
// 1 <= M <= 8, M taps <= 80, T >= 2.
long long wpe_ws_bytes(int B, int M, int T, int F, int taps);
hipError_t launch_wpe(const void* mix, const float* power, int B, int M, int T, int F, int taps, int delay, int iters,
                      double diag_load, double power_floor, void* out, void* ws, hipStream_t s);
hipError_t launch_wpe_debug(const void* ws, int B, int M, int F, int taps, void* g, int* fail, hipStream_t s);

// Online WPE (owpe.hip): the frame-recursive form, its state carried from call to call.  mix / out complex64
// [B][M][T][F], any T >= 1; the state holds fail int [B F], n int [B F], G complex128 [B F][M taps][M] and P complex128
// [B F][M taps][M taps], which launch_owpe_debug copies out, and the two rings.  1 <= M <= 8, M taps <= 80, delay >= 1,
// 0 <= context <= OWPE_CTX, owpe_lds_bytes(M, taps, delay) <= OWPE_LDS_LIMIT, B F < 2^31: the caller checks them.  owpe_init()
// once per device (the kernel's dynamic-LDS attribute).
constexpr int OWPE_CTX = 16, OWPE_LDS_LIMIT = 160 * 1024;
long long owpe_state_bytes(long long bins, int M, int taps, int delay);
long long owpe_lds_bytes(int M, int taps, int delay);
hipError_t owpe_init();
hipError_t launch_owpe_reset(void* state, int B, int M, int F, int taps, int delay, double init, hipStream_t s);
hipError_t launch_owpe(const void* mix, int B, int M, int T, int F, int taps, int delay, int context, double alpha,
                       double power_floor, void* out, void* state, hipStream_t s);
hipError_t launch_owpe_debug(const void* state, int B, int M, int F, int taps, int delay, void* g, void* p, int* fail, int* n,
                             hipStream_t s);

// Online AuxIVA (oiva.hip): the frame-recursive separation of the determined case, its state carried from
// call to call.  mix / est complex64 [B][M][T][F], images complex64 [B][M][M][T][F] or nullptr, any T >= 1; the state holds fail
// int [B F], n int [B F], W complex128 [B F][M][M] and V complex128 [B F][M][M][M], which launch_oiva_debug copies out.
// 2 <= M <= 8, 1 <= F <= 1025, B F < 2^31, 0 < alpha < 1: the caller checks them.  oiva_bins_per_pass(M): the bins one workgroup
// covers at once (-1 outside 2 .. 8).
long long oiva_state_bytes(long long bins, int M);
int oiva_bins_per_pass(int M);
hipError_t launch_oiva_reset(void* state, int B, int M, int F, double init, hipStream_t s);
hipError_t launch_oiva(const void* mix, int B, int M, int T, int F, int model, int ref_ch, double alpha, double floor, void* est,
                       void* images, void* state, hipStream_t s);
hipError_t launch_oiva_debug(const void* state, int B, int M, int F, void* w, void* v, int* fail, int* n, hipStream_t s);

// Online AuxIVA for K < M sources (overiva.hip): the frame-recursive overdetermined separation, its state
// carried from call to call.  mix complex64 [B][M][T][F], est complex64 [B][K][T][F], images complex64 [B][K][M][T][F] or nullptr,
// any T >= 1; the state holds fail int [B F], n int [B F], Ws complex128 [B F][K][M], J complex128 [B F][M - K][K], V complex128
// [B F][K][M][M] and C complex128 [B F][M][M], which launch_overiva_debug copies out.  2 <= M <= 8, 1 <= K <= M - 1, 1 <= F <=
// 1025, B F < 2^31, 0 < alpha < 1: the caller checks them.  overiva_bins_per_pass(M, K): the bins one workgroup covers at once
// (-1 outside those ranges).
long long overiva_state_bytes(long long bins, int M, int K);
int overiva_bins_per_pass(int M, int K);
hipError_t launch_overiva_reset(void* state, int B, int M, int K, int F, double init, hipStream_t s);
hipError_t launch_overiva(const void* mix, int B, int M, int K, int T, int F, int model, int ref_ch, double alpha, double floor,
                          void* est, void* images, void* state, hipStream_t s);
hipError_t launch_overiva_debug(const void* state, int B, int M, int K, int F, void* ws, void* jm, void* v, void* c, int* fail,
                                int* n, hipStream_t s);

// Online beamformer (obf.hip): the frame-recursive Souden MVDR / rank-1 MWF, its state carried from call to
// call.  mix complex64 [B][M][T][F], images complex64 [B][S][M][T][F], out complex64 [B][S][T][F], any T >= 1; the state holds fail
// int [B S F], n int [B S F], Phi_s and Phi_n complex128 [B S F][M][M] and w complex128 [B S F][M], which launch_obf_debug copies
// out.  2 <= M <= 8, 1 <= S <= 8, 1 <= F <= 1025, B S F < 2^31, 0 < alpha < 1, 0 <= ref_ch < M: the caller checks them.
// obf_cells_per_block(M): the cells (b, s, f) one workgroup covers (-1 outside 2 .. 8).
long long obf_state_bytes(long long cells, int M);
int obf_cells_per_block(int M);
hipError_t launch_obf_reset(void* state, int B, int S, int M, int F, double init, hipStream_t s);
hipError_t launch_obf(const void* mix, const void* images, int B, int S, int M, int T, int F, int noise, int ref_ch, double alpha,
                      double mu, double diag_load, double epsi, void* out, void* state, hipStream_t s);
hipError_t launch_obf_debug(const void* state, int B, int S, int M, int F, void* phi_s, void* phi_n, void* w, int* fail, int* n,
                            hipStream_t s);

// WPD convolutional beamformer (wpd.hip): one filter of order K = M (taps + 1) per (b, speaker, bin) from the
// observation and the source estimate, both read as launch_mvdr reads them (mix through a CView; the source through est /
// est_bstride / sel in pipeline mode or through src when est == nullptr), applied to the stacked observation and written through
// a COut.  The workspace holds fail int [B S F] and wbar complex128 [B S F][K] (order [y; z]), which launch_wpd_debug copies out.
// 2 <= M <= 8, taps >= 1, delay >= 1, K <= WPD_KMAX and wpd_lds_bytes(M, taps) <= 160 KB (true for every K <= WPD_KMAX),
// T > delay + taps - 1: the caller checks them.  wpd_init() once per device (the kernel's dynamic-LDS attribute).
constexpr int WPD_KMAX = 88;
struct WpdArgs {
  CView mix;
  const float* est;
  long long est_bstride;
  const int* sel;
  CView src;
  int S, B, F, M, T, Tp;
  int taps, delay, ref;
  double diag_load, power_floor;
};
long long wpd_ws_bytes(int B, int S, int F, int M, int taps);
int wpd_lds_bytes(int M, int taps);
hipError_t wpd_init();
hipError_t launch_wpd(const WpdArgs& a, const COut& out, void* ws, hipStream_t s);
hipError_t launch_wpd_debug(const void* ws, int B, int S, int F, int M, int taps, void* wbar, int* fail, hipStream_t s);

// Guided spatial clustering (cacgmm.hip): the cACGMM of K = S + 1 classes per (b, bin), started from and
// (prior "guided") held to the initial masks.  mix through a CView; init / masks float32 [B][K][F][T]; the refined source images
// gamma_s Y of the S speaker classes through a CImg (re == nullptr: not wanted), frames [T, Tp) written as zeros.  The
// workspace holds fail int [B F], the log-likelihood double [B F], pi double [B F][K] and B_k complex128 [B F][K][M][M], which
// launch_cacgmm_debug copies out.  2 <= M <= 8, 2 <= K <= 5, iters >= 0: the caller checks them.
// element (b, s, f, m, t) of the images at re[b*sb + s*ss + f*sf + m*sm + t*st], im likewise
struct CImg { float* re; float* im; long long sb, ss, sf, sm; int st, Tp; };
struct CacgmmArgs {
  CView mix;
  const float* init;
  float* masks;
  CImg img;
  int B, K, F, M, T;
  int iters, guided;
  double diag_load, prior_floor;
};
long long cacgmm_ws_bytes(int B, int K, int F, int M);
hipError_t launch_cacgmm(const CacgmmArgs& a, void* ws, hipStream_t s);
hipError_t launch_cacgmm_debug(const void* ws, int B, int K, int F, int M, void* bk, double* pi, double* ll, int* fail,
                               hipStream_t s);
// the initial masks of launch_cacgmm from S source estimates and the mixture: P_s = sum_m |est_s|^2, P_n = sum_m |y - sum_s est_s|^2,
// masks [B][S + 1][F][T] = P_k / sum_k P_k (1 / (S + 1) where that sum is 0).  The estimates as launch_mvdr reads them (est /
// est_bstride / sel in pipeline mode; src with the speaker stride src_ss when est == nullptr)
struct MaskArgs {
  CView mix;
  const float* est;
  long long est_bstride;
  const int* sel;
  CView src;
  long long src_ss;
  int S, B, F, M, T, Tp;
  float* masks;
};
hipError_t launch_masks_from_est(const MaskArgs& a, hipStream_t s);

// Joint multi-speaker beamformers (jbf.hip): LCMV, SDW-MWF and rank-1 MWF, one workgroup per (b, bin) that
// owns all S speakers.  mix through a CView; the S estimates as launch_masks_from_est reads them (est / est_bstride / sel in
// pipeline mode; src with the speaker stride src_ss when est == nullptr); out through a COut (os = the speaker stride), the
// frames [T, Tp) of it untouched.  The workspace holds fail int [B][S][F], w complex128 [B][S][F][M] and, for lcmv, the relative
// transfer functions d complex128 [B][S][F][M], which launch_jbf_debug copies out.  2 <= M <= 8, 1 <= S <= min(4, M), T >= 1,
// 0 <= ref < M: the caller checks them.
enum { JBF_LCMV = 0, JBF_MWF = 1, JBF_R1MWF = 2 };
struct JbfArgs {
  CView mix;
  const float* est;
  long long est_bstride;
  const int* sel;
  CView src;
  long long src_ss;
  int S, B, F, M, T, Tp;
  int kind;               // JBF_LCMV / JBF_MWF / JBF_R1MWF
  int noise_mix;          // lcmv: Phi_v from Y instead of Y - sum_s X_s ("LCMP")
  int rtf_eig;            // lcmv: a_s = the principal eigenvector of Phi_s instead of covariance whitening
  int ref;
  double mu, diag_load;
};
long long jbf_ws_bytes(int B, int S, int F, int M, int kind);
hipError_t launch_jbf(const JbfArgs& a, const COut& out, void* ws, hipStream_t s);
hipError_t launch_jbf_debug(const void* ws, int B, int S, int F, int M, int kind, void* w, void* d, int* fail, hipStream_t s);

// Blind separation (iva.hip): AuxIVA-ISS behind a per-bin PCA to K channels, projected back to the M
// microphones.  mix complex64 [B][F][M][T], images complex64 [B][S][F][M][T], order_out int [B][S] or nullptr.  The workspace
// holds fail int [B F], the eigenvectors and the projection complex128 [B F][M][K], power double [B][K], the chosen rows, phi
// double [B][K][T] and Y complex128 [B F][K][T], which launch_auxiva_debug copies out.  2 <= M <= 8, 1 <= S <= min(K, 4),
// K <= M, T >= 1, iters >= 0, 0 <= ref < M: the caller checks them.
struct IvaArgs {
  const void* mix;
  void* images;
  int* order_out;
  int B, S, K, F, M, T;
  int iters, laplace, ref;
  double floor;
};
long long iva_ws_bytes(int B, int K, int F, int M, int T);
int iva_resident_frames(int K);                    // the largest T the steering kernel keeps in registers
hipError_t launch_auxiva(const IvaArgs& a, void* ws, hipStream_t s);
hipError_t launch_auxiva_debug(const void* ws, int B, int K, int F, int M, int T, void* y, void* a, void* evec, double* power,
                               int* fail, hipStream_t s);

// Room simulator (room.hip): image-source RIRs of a shoebox and the scene mixer.  room double [B][3], beta
// double [B][6] (x0, x1, y0, y1, z0, z1), src double [B][S][3], mic double [B][M][3] -> rir double [B][S][M][Lh], fail int [B][S][M]
// (bit 0: bad geometry, bit 1: an image closer than 1e-3 m was dropped, bit 2: more than ROOM_MAX_IMAGES images or an N_i above
// ROOM_MAX_N; bits 0 and 2 leave a zero RIR).  The mixer: x float32 (b, s, j) at b xs[0] + s xs[1] + j xs[2], split int [B][S] or
// nullptr -> images, early (or nullptr) float32 [B][S][M][Lo], mix (or nullptr) float32 [B][M][Lo].  The caller checks the limits.
constexpr int ROOM_W = 80;                         // support of the fractional-delay kernel in samples
constexpr int ROOM_MAX_N = 255;                    // the largest image index per axis the static tables hold
constexpr double ROOM_MAX_IMAGES = 134217728.0;    // 2^27
constexpr int ROOM_MAX_B = 4096, ROOM_MAX_S = 4, ROOM_MAX_M = 16, ROOM_MAX_LH = 1 << 16, ROOM_MAX_L = 1 << 24;
int room_tile();                                   // taps / output samples per workgroup
hipError_t launch_room_rir(const double* room, const double* beta, const double* src, const double* mic, int B, int S, int M,
                           double fs, double c, int Lh, int max_order, double* rir, int* fail, hipStream_t s);
hipError_t launch_room_mix(const float* x, const long long* xs, const double* rir, const int* split /*[B][S] or nullptr*/, int B,
                           int S, int M, int L, int Lh, int Lo, float* images, float* early, float* mix, hipStream_t s);

// Source localisation (doa.hip): SRP, SRP-PHAT and MUSIC maps over a delay table, and their peaks.  mix
// complex64 [B][F][M][T], weight float32 [B][K][F][T] or nullptr (K = 1), tau double [Bg][D][M] (Bg 1 or B), pts double [D][3] ->
// q double [B][K][N][D], peak int / value double [B][K][N][S], fail int [B][K][N].  The workspace holds C complex128
// [B][K][N][F][M][M], the state of every bin and used / fail per map, which launch_doa_debug copies out.  block, hop and N are
// resolved (block >= 1, hop >= 1); the caller checks every limit.
constexpr int DOA_SRP = 0, DOA_SRP_PHAT = 1, DOA_MUSIC = 2;
constexpr int DOA_MAX_K = 8, DOA_MAX_S = 4, DOA_MAX_D = 65536;
struct DoaArgs {
  const float2* mix;
  const float* weight;
  const double* tau;
  const double* pts;
  int Bg, B, K, F, M, T, D;
  double fs;
  int kind, S, block, hop, N, f_lo, f_hi;
  double min_sep;
  double* q;
  int* peak;
  double* value;
  int* fail;
};
int doa_tile();                                    // candidates per workgroup of the steering kernel
int doa_bin_chunk();                               // bins per staged chunk of the steering kernel
long long doa_ws_bytes(long long B, long long K, long long N, long long F, long long M);
hipError_t launch_doa(const DoaArgs& a, void* ws, hipStream_t s);
hipError_t launch_doa_debug(const void* ws, int B, int K, int N, int F, int M, void* c, int* used, int* fail, hipStream_t s);

// source estimate of aligned speaker `spk` at microphone m: pointers to its frame row for bin f.  Args: MvdrArgs, WpdArgs,
// MaskArgs or JbfArgs (est / est_bstride / sel in pipeline mode, src when est == nullptr)
template <typename Args>
__device__ __forceinline__ void src_row(const Args& a, int b, int f, int m, int spk, const float*& re, const float*& im,
                                        int& st) {
  if (a.est) {
    const int n = b * a.M + m;
    const int q = a.sel ? a.sel[n * a.S + spk] : spk;
    const long long plane = (long long)a.F * a.Tp;
    const float* base = a.est + (long long)n * a.est_bstride + (long long)f * a.Tp;
    re = base + (long long)q * plane;
    im = base + (long long)(a.S + q) * plane;
    st = 1;
  } else {
    const long long off = (long long)b * a.src.sb + (long long)f * a.src.sf + (long long)m * a.src.sm;
    re = a.src.re + off;
    im = a.src.im + off;
    st = a.src.st;
  }
}

}  // namespace mn
