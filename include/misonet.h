/*
 * misonet.h -- C ABI of libmisonet_hip.so: the MI355X (gfx950) MISO1 -> MVDR -> MISO3 inference path.
 *
 * The reference (yuhogun0908/MISOnet) is pure Python and has no FFI layer; its boundary for this
 * path is the Python call surface named in SURVEY.md 8(b).  Each entry point below states the
 * reference interface it replaces (file:line into the reference tree).  All pointers named *_dev are
 * device pointers owned by the caller (e.g. torch tensors); the library allocates device memory only
 * in *_commit (weights).  Every call is asynchronous on the given HIP stream unless stated.  Return
 * value: 0 = success, negative = error (misonet_strerror / misonet_last_error).  One handle per
 * device; a handle is not re-entrant.
 *
 * Spectrogram layout at this boundary is the reference's: complex64 (interleaved re,im float32),
 * [B, channels, T frames, F = 129 bins], F innermost (model.py:77-80, tester.py:1025).
 */
#ifndef MISONET_H_
#define MISONET_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef struct misonet_net misonet_net;
typedef struct misonet_pipeline misonet_pipeline;
typedef void* misonet_stream;           /* hipStream_t */

enum {
  MISONET_OK = 0,
  MISONET_EINVAL = -1,        /* bad argument / unsupported geometry */
  MISONET_ESTATE = -2,        /* call order (e.g. forward before commit, missing tensor) */
  MISONET_EHIP = -3,          /* a HIP runtime call failed */
  MISONET_ENOMEM = -4,        /* workspace too small */
  MISONET_ENAN = -5           /* NaN in a network output (the reference drops into pdb, model.py:109-110) */
};

/* Geometry of one MISO trunk.  Mirrors the constructor arguments of MISO_1 / MISO_3
 * (model.py:9, 283): in_ch = 2*num_ch (MISO_1, model.py:16) or 2*(num_ch+2) (MISO_3, model.py:290);
 * out_ch = 2*num_spks (model.py:17); en_ch / de_ch = en/de_bottleneck_channels (config/NN_BSS.yml:120-123). */
typedef struct {
  int in_ch;
  int out_ch;
  int en_ch[7];
  int de_ch[7];
  int n_freq;                 /* must be 129 (nperseg 256): the encoder must reduce F to one bin */
  int tcn_norm;               /* ABI 400: `norm_type` of the constructors = the two OUTER norms of every TemporalBlock
                               * (model.py:530,535, chose_norm model.py:570-581): 0 "IN" (nn.InstanceNorm1d, no parameters;
                               * config/NN_BSS.yml:123), 1 "gLN" (GlobalLayerNorm: gamma, beta), 2 "cLN"
                               * (ChannelwiseLayerNorm: gamma, beta), 3 anything else (nn.BatchNorm1d in eval mode: weight,
                               * bias, running_mean, running_var).  The 2-D blocks hard-code InstanceNorm2d (model.py:413,430)
                               * and the norm inside DepthwiseSeparableConv is always gLN (model.py:533,537). */
} misonet_cfg;

const char* misonet_strerror(int code);
const char* misonet_last_error(void);   /* thread-local detail of the last failing call */
int misonet_version(void);

/* ---- network handle: replaces nn.Module construction + load_state_dict (run.py:121-151) --------------- */
int misonet_net_create(const misonet_cfg* cfg, misonet_net** out);
int misonet_net_destroy(misonet_net* net);
/* the state_dict this network expects: the reference's key names (268 tensors for the default cfg) */
int misonet_net_num_tensors(const misonet_net* net);
const char* misonet_net_tensor_name(const misonet_net* net, int i);
long long misonet_net_tensor_numel(const misonet_net* net, int i);
/* host float32 data of one state_dict entry (load_state_dict, run.py:139-151) */
int misonet_net_set_tensor(misonet_net* net, const char* key, const float* host_data, long long numel);
/* all tensors set -> repack into the kernel layouts and upload to the current device (synchronous) */
int misonet_net_commit(misonet_net* net);

/* arithmetic of the 3x3 convolutions (99.4 % of the FLOPs; the reference computes them in float32, model.py:77-80,
 * 401-482):
 *   0 "f32"     exact float32 matrix cores (v_mfma_f32_32x32x2_f32, bitwise an fmaf chain);
 *   3 "bf16x6"  (the DEFAULT of a new handle, and what bench.py reports) fp32-FAITHFUL on the bf16 matrix cores: both operands are represented exactly as three bf16 pieces
 *               (24 bits), the six leading partial products are accumulated in float32 (the dropped ones are < 2^-23
 *               of a product, one float32 rounding); activations travel pre-split (oct3 layout: hi | mid | lo, 8 channels
 *               per 16-byte unit), the instance norm is folded into per-sample weights, staging is LDS-DMA.  Same error
 *               against the reference as mode 0 (2.3e-6 per forward) at 1.65 x its speed;
 *   5 "f32w"    (ABI 430) mode 0 with the DenseBlock convs (model.py:437-482: 94 % of the MACs) in Winograd F(2x2, 3x3) form:
 *               float32 products and sums on the same matrix cores, 2.25 x fewer of them (conv_wino.hip); measured 2.0e-6
 *               per forward against the reference (mode 0: 2.6e-6), 1.47 x mode 0's speed.  Same planar float32 layout.
 * The numbers 1, 2 ("bf16x3": 16-bit operands), 4 ("f16x3": 22-bit operands) and 6 ("bf16x6w", ABI 440: the Winograd form in mode
 * 3's arithmetic -- correct, 0.8 x mode 3's speed) belonged to alternatives that were measured and dropped (ABI 450; LAB.md): the
 * library answers MISONET_EINVAL to them.
 * The choice is internal to the workspace (whose size depends on it: misonet_net_workspace_bytes must be asked again
 * after a change): inputs, outputs and taps are the same float32 / complex64 tensors in every mode. */
int misonet_net_set_precision(misonet_net* net, int mode);
int misonet_net_get_precision(const misonet_net* net);

/* workspace (device bytes) for n_samples spectrograms of n_frames frames */
long long misonet_net_workspace_bytes(const misonet_net* net, int n_samples, int n_frames);

/* MISO_1.forward(mixture) (model.py:76-111) and MISO_3.forward(mixture, a, b) (model.py:350-395).
 * The input is given as n_seg channel segments, each complex64 [B, seg_ch[i], T, F]; their real parts are
 * concatenated in order, then their imaginary parts (model.py:80 / 360-364).  MISO_1: one segment (mixture);
 * MISO_3: three (mixture, a, b).  out_dev: complex64 [B, out_ch/2, T, F]. */
int misonet_net_forward(misonet_net* net, int n_seg, const void* const* seg_dev, const int* seg_ch,
                        int B, int T, void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* synchronises the stream and reports MISONET_ENAN if the last forward on this workspace produced a NaN */
int misonet_net_check(misonet_net* net, const void* ws_dev, misonet_stream stream);

/* Workspace liveness: by default activation buffers whose lifetimes do not overlap share memory (the only cross-level
 * lifetime of the reference is the skip list xs, model.py:84-99): 0.26 GB per forward-sample at T = 1001 in mode 3
 * instead of 0.55.  keep != 0 gives every buffer its own memory so that every tap below stays readable after a forward;
 * the workspace size changes (ask misonet_net_workspace_bytes again). */
int misonet_net_keep_activations(misonet_net* net, int keep);
/* diagnostic (host only, no GPU): the memory plan of ONE sample's activation block for n_frames frames -- per buffer its
 * byte offset inside the block, its size and the first / last step of a forward at which it is alive (0 input written,
 * 1 + b encoder b, 8 TCN, 9 + i decoder i, 16 results read).  Returns the number of buffers written (<= max_buffers) or
 * a negative error.  tests/test_lib_abi.py checks that buffers alive at the same step never overlap. */
int misonet_net_buffer_plan(const misonet_net* net, int n_frames, int max_buffers, long long* offset_bytes,
                            long long* size_bytes, int* first_step, int* last_step);
/* diagnostic (host only, no GPU; ABI 470): which kernel runs each of the network's 3x3 conv layers in precision mode `mode` --
 * the encoder stack, then the decoder stack, in launch order (64 layers).  The choice is made once, when the net is created,
 * from the layer shapes alone; a forward launches exactly these kernels or fails (there is no fall-back).  kind[i]:
 * 0 DIRECT (conv3x3_mfma, exact f32), 1 W1D (the same kernel in 1-D Winograd form along T), 2 FEW (conv3x3_few), 3 WINO
 * (conv3x3_wino_f32), 4 X6_FIRST (conv3x3_x6_first), 5 X6 (conv3x3_bf16x6).
 * Returns the number of layers written (<= max_layers), or MISONET_EINVAL for a mode the library does not have. */
int misonet_net_conv_plan(const misonet_net* net, int mode, int max_layers, int* kind);
/* test/diagnostic taps: copy an intermediate activation of the LAST forward (still in ws_dev) out as float32
 * [B, C, T, F] in the reference's layout and normalisation.  Names: enc0_conv, enc0..enc6, tcn_out, dec0..dec6.
 * Needs misonet_net_keep_activations(net, 1) BEFORE that forward (MISONET_ESTATE otherwise), except dec6 (the output). */
int misonet_net_tap_shape(const misonet_net* net, const char* name, int* C, int* F);
int misonet_net_tap(misonet_net* net, const char* name, const void* ws_dev, int B, int T, float* dst_dev,
                    misonet_stream stream);

/* ---- beamforming: Tester_Enhance.Apply_Beamforming(source_stft, mix_stft, epsi) (tester.py:1071-1136) and the
 * settings its author kept beside it (MPDR, conditioning, trace normalisation, BAN; GEV from the nn-gev family) ---- */
/* src_dev, mix_dev: complex64 [B, F, M, T] contiguous (the reference passes permuted views, tester.py:921-923);
 * out_dev: complex64 [B, T, F] (tester.py:1134).  2 <= M <= 8.  misonet_mvdr is the reference's live path: residual-noise
 * MVDR, steering vector from the principal eigenvector of Phi_s, sequential phase correction, eps I loading. */
long long misonet_mvdr_workspace_bytes(int B, int F, int M);
int misonet_mvdr(const void* src_dev, const void* mix_dev, int B, int F, int M, int T, float epsi,
                 void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_mvdr, copy steering vectors (after phase correction) and beamformer weights,
 * both complex128 [B,F,M], to device buffers (either may be NULL) */
int misonet_mvdr_debug(const void* ws_dev, int B, int F, int M, void* steer_c128_dev, void* w_c128_dev,
                       misonet_stream stream);

/* ---- selectable beamformers (ABI 510) ------------------------------------------------------------------------------
 * Phi_s = S S^H / T and Phi_n = N N^H / T are accumulated, made Hermitian and divided by T as above (tester.py:1091-1100);
 * everything after the reduced covariances is float64, per bin, without atomics: bit-reproducible and independent of B.
 *   noise            0 "residual": N = Y - S (tester.py:1095);  1 "mix": N = Y (tester.py:1096: MPDR, "MP-GEV")
 *   condition        gamma >= 0: Phi_n <- (Phi_n + gamma tr(Phi_n) / M I) / (1 + gamma), PER BIN (equation 2.3 of the paper
 *                    that tester.py:1170 cites; the reference's dead code takes the trace of a whole [F, M, M] slab)
 *   trace_normalize  Phi_n <- Phi_n / tr(Phi_n) (tester.py:1099), after the conditioning
 *   epsi             Phi_n' = Phi_n + epsi I, last (tester.py:1221)
 *   kind             0 "mvdr": the solve of misonet_mvdr: d from Phi_s, d / d[0], sqrt(M / ||d||), phase correction along f,
 *                      w = Phi_n'^-1 d / (d^H Phi_n'^-1 d);
 *                    1 "souden": G = Phi_n'^-1 Phi_s, w = G[:, ref_ch] / tr(G); w = 0 where tr(G) == 0;
 *                    2 "gev": the eigenvector of the largest lambda in Phi_s w = lambda Phi_n' w (Cholesky Phi_n' = L L^H,
 *                      C = L^-1 Phi_s L^-H, cyclic Jacobi on C, w = L^-H u), scaled to w^H Phi_n' w = 1 and rotated PER BIN so
 *                      that (Phi_n' w)[ref_ch] is real and >= 0 (left as it is where that entry is 0).  A Cholesky pivot that
 *                      is not positive gives a non-finite w; nothing is clamped.
 *   ban              w <- w sqrt|w^H Phi_n' Phi_n' w| / |w^H Phi_n' w| (tester.py:1196-1208 with eps = 0); w stays where the
 *                    denominator is 0
 *   ref_ch           0 <= ref_ch < M: the reference microphone of "souden" and "gev"
 * With the defaults of misonet_bf_opts_default every output bit of misonet_beamform is that of misonet_mvdr.
 * Bad fields (unknown kind or noise, negative or non-finite condition or epsi, ref_ch outside [0, M)) are refused on the
 * host with MISONET_EINVAL and a message (the size function: -1), before any launch. */
typedef struct {
  int kind;
  int noise;
  double condition;
  int trace_normalize;
  float epsi;
  int ban;
  int ref_ch;
} misonet_bf_opts;
int misonet_bf_opts_default(misonet_bf_opts* opts);      /* mvdr, residual, 0, 0, 1e-6f, 0, 0 */
long long misonet_beamform_workspace_bytes(int B, int F, int M, const misonet_bf_opts* opts);
int misonet_beamform(const void* src_dev, const void* mix_dev, int B, int F, int M, int T, const misonet_bf_opts* opts,
                     void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_beamform, copy the weights w complex128 [B, F, M] and, for "gev", lambda_max float64 [B, F]
 * (MISONET_EINVAL for lambda of another kind) to device buffers (either may be NULL).  For "mvdr" misonet_mvdr_debug reads
 * the same workspace. */
int misonet_beamform_debug(const void* ws_dev, int B, int F, int M, const misonet_bf_opts* opts, void* w_c128_dev,
                           double* lambda_dev, misonet_stream stream);

/* ---- WPE dereverberation (ABI 520) ---------------------------------------------------------------------------------
 * Weighted prediction error (Nakatani et al. 2010; Yoshioka & Nakatani 2012), per (item b, bin f), independent of every other;
 * Y = mix[b, :, :, f] is [M, T]:
 *   Z[(k M + m), t] = Y[m, t - delay - k]   (k = 0 .. taps - 1; zero for t - delay - k < 0), order N = M taps
 *   X <- Y; repeat `iterations` times:
 *     p[t] = mean_m |X[m, t]|^2                  (first iteration: power_dev[b, t, f] when given -- "DNN-WPE")
 *     w[t] = 1 / max(p[t], power_floor max_t p[t])
 *     R = sum_t w[t] Z[:, t] Z[:, t]^H,  P = sum_t w[t] Z[:, t] Y[:, t]^H,  R += diag_load tr(R) / N I
 *     G = R^-1 P  (Cholesky R = L L^H, two triangular solves),  X = Y - G^H Z
 * With the defaults this is nara_wpe's wpe_v8 with psd_context = 0.  Everything after the complex64 loads is float64 (the
 * correlations on the float64 matrix pipe); X is rounded to complex64 once, on the final store.  Every sum runs in a fixed
 * order, without atomics: the bits of an item depend neither on B nor on its position in the batch.
 * A bin in which a Cholesky pivot is not finite or not > 0 (the all-zero bin) is passed through unchanged -- X = Y, the
 * remaining iterations skipped, fail[b, f] = 1, G = 0 -- and nothing is clamped.
 * mix_dev and out_dev are complex64 [B, M, T, F], the output layout of misonet_stft and the input layout of misonet_istft;
 * they must not be the same buffer.  Any T >= 2 (a whole recording is one call), 1 <= M <= 8, M taps <= 80, delay >= 1,
 * 1 <= iterations <= 10, diag_load and power_floor finite and >= 0: anything else is refused on the host with MISONET_EINVAL
 * and a message (the size function: -1), before any launch; a short workspace is MISONET_ENOMEM. */
typedef struct {
  int taps;
  int delay;
  int iterations;
  double diag_load;
  double power_floor;
} misonet_wpe_opts;
int misonet_wpe_opts_default(misonet_wpe_opts* opts);    /* 10, 3, 3, 0.0, 1e-10 */
long long misonet_wpe_workspace_bytes(int B, int M, int T, int F, const misonet_wpe_opts* opts);
int misonet_wpe(const void* mix_dev, const float* power_dev, int B, int M, int T, int F, const misonet_wpe_opts* opts,
                void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_wpe, copy the filter G of the last iteration, complex128 [B, F, M taps, M], and fail int32 [B, F]
 * to device buffers (either may be NULL) */
int misonet_wpe_debug(const void* ws_dev, int B, int M, int F, const misonet_wpe_opts* opts, void* g_c128_dev, int* fail_dev,
                      misonet_stream stream);

/* ---- WPD (ABI 530) ---------------------------------------------------------------------------------------------------
 * The weighted power minimisation distortionless response convolutional beamformer (Nakatani & Kinoshita 2019) in the
 * mask-based form of Zhang, Boeddeker et al. 2020 (ESPnet's "wpd"): one filter per (item b, bin f) that dereverberates and
 * beamforms in one solve, driven by the power of the SOURCE estimate.  Y = mix[b, f] and S = src[b, f] are [M, T]:
 *   Z[(k M + m), t] = Y[m, t - delay - k]   (k = 0 .. taps - 1; zero before the start: WPE's Z)
 *   ybar[t] = [Y[:, t]; Z[:, t]], order K = M (taps + 1)
 *   p[t] = mean_m |S[m, t]|^2,  w[t] = 1 / max(p[t], power_floor max_t p[t])
 *   R = sum_t w[t] ybar[t] ybar[t]^H,  R += diag_load tr(R) / K I
 *   Phi_s = S S^H / T (Hermitian, as misonet_beamform makes it), Phibar = Phi_s in the top-left block of a K x K zero matrix
 *   A = R^-1 Phibar (Cholesky R = L L^H, two triangular solves),  wbar = A[:, ref_ch] / tr(A)  (the complex trace, as "souden")
 *   out[t] = wbar^H ybar[t]
 * One pass: p is not re-estimated from the output, and there is no steering-vector form.  Everything after the complex64 loads is
 * float64 (the correlations on the float64 matrix pipe); out is rounded to complex64 once, on the store.  Every sum runs in a
 * fixed order, without atomics: the bits of a bin depend neither on B nor on its position in the batch (nor, in the fused
 * pipeline, on the number of speakers).
 * A (b, f) FAILS if a Cholesky pivot is not finite or not > 0 (the all-zero bin or source: w infinite, R not finite) or if tr(A) is
 * not finite or is 0: then wbar = 0, out = 0 and fail[b, f] = 1.  Nothing is clamped.
 * src_dev, mix_dev, out_dev: the layouts of misonet_beamform (complex64 [B, F, M, T] and [B, T, F]).  2 <= M <= 8, taps >= 1,
 * delay >= 1, K = M (taps + 1) <= 88 (the order the Gram scheme reaches; its K x K factor, right-hand sides and frame windows take
 * 156 KB of the 160 KB of LDS at M = 8, taps = 10), T > delay + taps - 1, 0 <= ref_ch < M, diag_load and power_floor finite and
 * >= 0: anything else is refused on the host with MISONET_EINVAL and a message (the size function: -1), before any launch and
 * before any pointer is looked at; a short workspace is MISONET_ENOMEM.  The call allocates nothing and does not synchronise (its
 * first use on a device sets one kernel attribute). */
typedef struct {
  int taps;
  int delay;
  double diag_load;
  double power_floor;
  int ref_ch;
} misonet_wpd_opts;
int misonet_wpd_opts_default(misonet_wpd_opts* opts);    /* 5, 3, 0.0, 1e-10, 0 */
long long misonet_wpd_workspace_bytes(int B, int F, int M, const misonet_wpd_opts* opts);
int misonet_wpd(const void* src_dev, const void* mix_dev, int B, int F, int M, int T, const misonet_wpd_opts* opts,
                void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_wpd, copy wbar complex128 [B, F, K] (order [y; z]: the M weights on the current frame first) and
 * fail int32 [B, F] to device buffers (either may be NULL) */
int misonet_wpd_debug(const void* ws_dev, int B, int F, int M, const misonet_wpd_opts* opts, void* wbar_c128_dev, int* fail_dev,
                      misonet_stream stream);

/* ---- guided spatial clustering: cACGMM (ABI 560) ------------------------------------------------------------------------
 * The complex angular central Gaussian mixture model (Ito, Araki & Nakatani 2016) that mask-based front ends put between a
 * network and a beamformer ("guided source separation"): the time-frequency masks are re-estimated from the observation itself,
 * started from -- and, with prior 1, held to -- the masks the caller brings.  This is the project's own definition in that
 * family (INTEGRATION.md 4l has it in full; tests/cacgmm_ref.py restates it); nothing here was compared against pb_bss.
 * Per (item b, bin f), K = S + 1 classes (k < S: speaker k; S: noise), Y = mix[b, f] [M, T], everything after the loads float64:
 *   z[t] = y[t] / |y[t]|; a frame with |y[t]|^2 == 0 is EMPTY: it enters no sum, its output mask is its initial mask
 *   sweep 0 (M-step only, gamma = the initial masks, q = 1):
 *     n_k = sum_t gamma[k, t],  B_k = M / n_k sum_t gamma[k, t] / q[k, t] z[t] z[t]^H,  B_k += diag_load tr(B_k) / M I,
 *     B_k = L_k L_k^H (Cholesky), logdet_k = 2 sum_i log L_k[i, i]
 *     prior 0 "bin": pi[k] = n_k / sum_k n_k;  prior 1 "guided": pi[k, t] = max(initial mask[k, t], prior_floor), fixed
 *   iteration 1 .. iterations (E-step, then the M-step above; the last one the E-step only):
 *     q[k, t] = |L_k^-1 z[t]|^2,  l[k, t] = log pi - logdet_k - M log q[k, t],  gamma[., t] = softmax_k l[., t]
 *   log-likelihood = sum_t logsumexp_k l[k, t] of the last E-step; iterations == 0 returns the initial masks
 * A bin is UNSOLVED when an n_k is not > 0 or not finite, a Cholesky pivot is not finite or not > 0, or the log-likelihood of an
 * E-step is not finite: it keeps its initial masks (and their images), fail[b, f] = 1.  Nothing is clamped.  Every sum runs in
 * a fixed order, without atomics: the bits of a bin depend neither on B nor on its position in the batch.
 * mix_dev complex64 [B, F, M, T] (the layout of misonet_beamform); init_masks_dev, masks_out_dev float32 [B, K, F, T] (two
 * different buffers); images_out_dev NULL or complex64 [B, S, F, M, T] = gamma_s Y rounded once, speaker s in the layout
 * misonet_beamform and misonet_wpd take as src_dev.  2 <= M <= 8, 2 <= K <= 5 (1 <= S <= 4), T >= 1, 0 <= iterations <= 1000,
 * diag_load and prior_floor finite and >= 0, prior_floor > 0 with prior 1: anything else is MISONET_EINVAL with a message (the size
 * function: -1) before any launch and before any pointer is looked at; a short workspace is MISONET_ENOMEM.  The workspace does
 * not grow with T.  The calls allocate nothing and do not synchronise. */
typedef struct {
  int iterations;
  int prior;               /* 0 "bin", 1 "guided" */
  double diag_load;
  double prior_floor;
} misonet_cacgmm_opts;
int misonet_cacgmm_opts_default(misonet_cacgmm_opts* opts);    /* 10, 0, 1e-8, 1e-6 */
long long misonet_cacgmm_workspace_bytes(int B, int K, int F, int M);
int misonet_cacgmm(const void* mix_dev, const float* init_masks_dev, int B, int K, int F, int M, int T,
                   const misonet_cacgmm_opts* opts, float* masks_out_dev, void* images_out_dev, void* ws_dev, long long ws_bytes,
                   misonet_stream stream);
/* diagnostic: after misonet_cacgmm, copy B_k of the last M-step (as it was factored) complex128 [B, F, K, M, M], the bin prior
 * n_k / sum n_k of that M-step float64 [B, F, K] (computed for either prior), the log-likelihood float64 [B, F] and fail int32
 * [B, F] to device buffers (any may be NULL).  An unsolved bin and iterations == 0 report zeros for the first three. */
int misonet_cacgmm_debug(const void* ws_dev, int B, int K, int F, int M, void* bk_c128_dev, double* pi_dev, double* ll_dev,
                         int* fail_dev, misonet_stream stream);
/* initial masks from S source estimates est_dev complex64 [B, S, F, M, T] and mix_dev [B, F, M, T]: P_s = sum_m |est_s|^2,
 * P_n = sum_m |y - sum_s est_s|^2 (float64), masks_out_dev float32 [B, S + 1, F, T] = P_k / sum_k P_k, 1 / (S + 1) where that sum is 0 */
int misonet_masks_from_estimates(const void* est_dev, const void* mix_dev, int B, int S, int F, int M, int T,
                                 float* masks_out_dev, misonet_stream stream);

/* ---- joint multi-speaker beamformers: LCMV, SDW-MWF, rank-1 MWF (ABI 570) ----------------------------------------------------
 * The beamformers above see one source estimate and the mixture; these own a whole bin, all S speakers at once: "lcmv" (unit
 * gain on the target, a null on every other speaker), "mwf" / "sdw_mwf" and "r1mwf" of the mask-based family, with an explicit
 * interference model.  This is the project's own definition in the ESPnet / pb_bss family (INTEGRATION.md 4m has it in full;
 * tests/jbf_ref.py restates it in NumPy float64); nothing here was compared against those packages and no quality figure on real
 * speech was measured.
 * Per (item b, bin f): Y = mix[b, f] [M, T], X_s = src[b, s, f] [M, T], complex64 as loaded, float64 after the loads:
 *   V = Y - sum_s X_s,  Phi_s = X_s X_s^H / T,  Phi_v = V V^H / T  (noise 1 "mix", lcmv only: Y Y^H / T, power minimisation, "LCMP")
 *   (the lower triangle computed and mirrored, a real diagonal),  R = Phi_v + diag_load tr(Phi_v) / M I,  N_s = sum_{j != s} Phi_j + R
 *   kind 0 "lcmv":  R = L L^H (Cholesky), once per bin;
 *                   rtf 0 "cw" (covariance whitening): C_s = L^-1 Phi_s L^-H, q_s = its principal eigenvector (cyclic complex
 *                   Jacobi), a_s = L q_s;  rtf 1 "eig": a_s = the principal eigenvector of Phi_s;
 *                   d_s = a_s / a_s[ref_ch],  D = [d_0 .. d_{S-1}],  Z = L^-1 D,  G = Z^H Z = K K^H (Cholesky),
 *                   W = L^-H Z G^-1,  w_s = column s of W, so that w_s^H d_j = delta_sj.  With S = 1 this is the MVDR
 *                   w = R^-1 d / (d^H R^-1 d).  mu is ignored.
 *   kind 1 "mwf":   w_s = (Phi_s + mu N_s)^-1 Phi_s e_ref  (Cholesky; mu > 0; mu = 1: the multichannel Wiener filter)
 *   kind 2 "r1mwf": A_s = N_s^-1 Phi_s (Cholesky of N_s),  w_s = A_s e_ref / (mu + tr A_s)  (mu >= 0; the complex trace, as
 *                   "souden").  mu = 0: the Souden MVDR on the sum-of-sources model; with S = 1 that is "souden" with noise
 *                   "residual", condition = diag_load, epsi = 0.  For S > 1 it differs from "souden" by the cross terms X_j V^H
 *                   that the residual (Y - X_s)(Y - X_s)^H carries and the sum-of-sources model leaves out.
 *   out_s[t] = w_s^H y[t], rounded to complex64 once, on the store.
 * Nothing is clamped.  "lcmv" FAILS as a whole bin -- a pivot of R or of G not finite or not > 0, a tr Phi_s that is 0 or not
 * finite (an exactly-zero estimate has no direction), an a_s[ref_ch] that is 0 or not finite: w_s = 0, out_s = 0 and
 * fail[b, s, f] = 1 for every s.  "mwf" / "r1mwf" fail per (b, s, f) -- a pivot, for "r1mwf" also mu + tr A_s 0 or not finite --
 * and only that speaker is zeroed and flagged; a zero Phi_s under "mwf" is no failure (w_s = 0, fail = 0, as "souden").  Equal
 * leading eigenvalues make d_s arbitrary: that case is NOT detected.  Every sum runs in a fixed order, without atomics: the bits
 * of a bin depend neither on B nor on its position in the batch (on S they depend by definition).
 * src_dev complex64 [B, S, F, M, T] (speaker s in the layout misonet_beamform takes), mix_dev complex64 [B, F, M, T], out_dev
 * complex64 [B, S, T, F].  2 <= M <= 8, 1 <= S <= 4, S <= M, T >= 1, 0 <= ref_ch < M, diag_load finite and >= 0, mu finite and
 * > 0 for "mwf", >= 0 for "r1mwf"; noise 1 and rtf 1 belong to "lcmv" and must be 0 elsewhere: anything else is MISONET_EINVAL
 * with a message (the size function: -1) before any launch and before any pointer is looked at; a short workspace is
 * MISONET_ENOMEM.  The workspace does not grow with T.  The calls allocate nothing and do not synchronise. */
typedef struct {
  int kind;                /* 0 "lcmv", 1 "mwf", 2 "r1mwf" */
  int noise;               /* 0 "residual", 1 "mix" (lcmv only) */
  int rtf;                 /* 0 "cw", 1 "eig" (lcmv only) */
  double mu;
  double diag_load;
  int ref_ch;
} misonet_jbf_opts;
int misonet_jbf_opts_default(misonet_jbf_opts* opts);    /* 0, 0, 0, 1.0, 0.0, 0 */
long long misonet_beamform_joint_workspace_bytes(int B, int S, int F, int M, const misonet_jbf_opts* opts);
int misonet_beamform_joint(const void* src_dev, const void* mix_dev, int B, int S, int F, int M, int T,
                           const misonet_jbf_opts* opts, void* out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_beamform_joint, copy the weights complex128 [B, S, F, M], the relative transfer functions d_s
 * complex128 [B, S, F, M] ("lcmv" only: MISONET_EINVAL for another kind) and fail int32 [B, S, F] to device buffers (any may be
 * NULL).  A failed speaker reports zeros for the first two. */
int misonet_beamform_joint_debug(const void* ws_dev, int B, int S, int F, int M, const misonet_jbf_opts* opts, void* w_c128_dev,
                                 void* rtf_c128_dev, int* fail_dev, misonet_stream stream);

/* ---- blind separation: AuxIVA (ABI 580) -------------------------------------------------------------------------------------
 * A front end that needs no weights: auxiliary-function independent vector analysis with iterative source steering (AuxIVA-ISS;
 * Ono 2011, Scheibler & Ono 2020), inverse-free, behind a per-bin PCA to K channels and projected back to all microphones by
 * least squares.  Its images have the layout of the source estimates every beamformer above and the cACGMM consume.  This is the
 * project's own definition in the pyroomacoustics / torchiva family (INTEGRATION.md 4n has it in full; tests/iva_ref.py restates
 * it in NumPy float64); nothing here was compared against those packages.
 * mix complex64 [B, F, M, T]; float64 after the loads; every recording b on its own; K = channels (0: K = S):
 *   0. a bin (b, f) that holds a non-finite sample: fail |= 1, the bin is all zero in every step below, its images are 0
 *   1. PCA per bin: R = X X^H / T, its eigenvectors by the cyclic complex Jacobi of the beamformers, eigenvalues descending (equal
 *      ones: the lower index first), each eigenvector rotated so that its ref_ch component is real and >= 0 (left as it is when
 *      that component is 0); an eigenvalue not above 1e-12 times the largest counts as 0 and its eigenvector (also in the diagnostic
 *      export) is 0: a bin of lower rank than K -- T < K, dead or identical microphones, a zero bin -- has no such direction, its row
 *      of Z is 0 in exact arithmetic, and the rounding noise that would stand there is not scaled up to a source;
 *      Z = E_K^H X [K, T] (no whitening), Y = Z
 *   2. per iteration, once, from the Y of all bins, the sum over f ascending:
 *        model 0 "gauss":   phi_k[t] = 1 / max(1 / F sum_f |y_k[f, t]|^2, floor)
 *        model 1 "laplace": phi_k[t] = 1 / max(2 sqrt(sum_f |y_k[f, t]|^2), floor)
 *   3. per iteration and bin, for s = 0 .. K - 1 in order, y_s the row as it stands before the step:
 *        num_k = sum_t phi_k[t] y_k[t] conj(y_s[t]),  den_k = sum_t phi_k[t] |y_s[t]|^2
 *        k != s: v_k = num_k / den_k (0 when den_k = 0);  d = den_s / T, v_s = 1 - 1 / sqrt(d) (0 when d = 0)
 *        y_k <- y_k - v_k y_s for all k;  a non-finite v_k is replaced by 0 and the bin gets fail |= 2
 *   4. after the last iteration: A[f, m, k] = sum_t x_m[t] conj(y_k[t]) / sum_t |y_k[t]|^2 (0 when the denominator is 0),
 *      power_k = sum_{f, t} |A[f, ref_ch, k] y_k[f, t]|^2, order = the S rows of largest power, descending (ties: the lower
 *      index), images[b, s, f, m, t] = A[f, m, order_s] y_{order_s}[f, t], rounded once to complex64
 * iterations = 0: steps 1 and 4 only.  Every sum over t runs in a fixed order, without atomics: the bits of a recording depend
 * neither on B nor on its position in the batch.  One launch sequence on the stream (3 + 2 iterations kernels), no host
 * synchronisation, no allocation: it can be captured in a HIP graph.  Up to misonet_auxiva_resident_frames(K) frames a bin's Y stays
 * in registers through the K source steps of an iteration; beyond that it is walked in the workspace.
 * 2 <= M <= 8, 1 <= S <= min(M, 4), S <= K <= M, B, F, T >= 1, 0 <= iterations <= 1000, floor finite and > 0, 0 <= ref_ch < M:
 * anything else is MISONET_EINVAL with a message (the size function: -1) before any launch and before any pointer is looked at; a
 * short workspace is MISONET_ENOMEM.  The workspace grows with T (it holds Y as complex128 [B, F, K, T]). */
typedef struct {
  int iterations;
  int model;               /* 0 "gauss", 1 "laplace" */
  int channels;            /* K; 0 = S */
  int ref_ch;
  double floor;
} misonet_iva_opts;
int misonet_iva_opts_default(misonet_iva_opts* opts);    /* 20, 0, 0, 0, 1e-10 */
long long misonet_auxiva_workspace_bytes(int B, int S, int K, int F, int M, int T);    /* -1 on bad arguments */
int misonet_auxiva_resident_frames(int K);
/* images_out_dev complex64 [B, S, F, M, T]; order_out_dev int32 [B, S] (the chosen rows of Y) or NULL */
int misonet_auxiva(const void* mix_dev, int B, int S, int F, int M, int T, const misonet_iva_opts* opts, void* images_out_dev,
                   int* order_out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_auxiva, copy Y complex128 [B, F, K, T], A complex128 [B, F, M, K], the eigenvectors E_K complex128
 * [B, F, M, K], power float64 [B, K] and fail int32 [B, F] to device buffers (any may be NULL) */
int misonet_auxiva_debug(const void* ws_dev, int B, int K, int F, int M, int T, void* y_c128_dev, void* a_c128_dev,
                         void* evec_c128_dev, double* power_dev, int* fail_dev, misonet_stream stream);

/* ---- PIT speaker alignment (tester.py:1043-1065 and 889-915) ----------------------------------------------- */
/* anchor_dev, cand_dev: complex64 [B, S, T, F]; sel_dev: int32 [B, S] with aligned speaker i = cand[sel[i]];
 * dist_dev (required: it is the call's only scratch, so the call allocates nothing and stays asynchronous): float64,
 * B*S*S*(F+1) elements.  The first [B, S, S] receive dist[i][j] = sum_{t,f} | |anchor_i| - |cand_j| |; the rest holds
 * the per-bin partial sums [B, F, S, S], which are added in bin order (no atomics: the distances and the selected
 * permutation are bit-reproducible from run to run).  All S! permutations are enumerated in
 * itertools.permutations order with the first minimum winning, as the reference's einsum('bij,pij->bp') + argmin
 * (tester.py:1053-1064); 1 <= S <= 4.
 * dist_bytes = the size of dist_dev in bytes: less than misonet_pit_scratch_bytes(B, S, F) returns MISONET_ENOMEM (ABI 400;
 * until ABI 300 the size was implicit, and it had grown from B*S*S doubles in ABI 200 without the signature changing). */
long long misonet_pit_scratch_bytes(int B, int S, int F);
int misonet_pit_select(const void* anchor_dev, const void* cand_dev, int B, int S, int T, int F,
                       int* sel_dev, double* dist_dev, long long dist_bytes, misonet_stream stream);

/* ---- continuous separation: a long recording in overlapping windows without clean references (ABI 460) -------------
 * Window k of the recording covers samples [kH, kH + W) (64 | W, 64 | H, W/2 <= H <= W - 256); each window goes through
 * misonet_pipeline_run_wav with clean_dev == NULL.  The speaker order of window k is linked to window k-1 through their
 * T - H/64 shared frames, and the windows' waveforms are joined by a raised-cosine cross-fade over the overlap ov = W - H.
 *
 * misonet_css_align: est_dev complex64 [K, S, T, F] = K consecutive windows hop_frames = H/64 frames apart.
 *   D_k[i][j] = sum_{t < T - hop_frames} sum_f | |est[k-1, i, t + hop_frames, f]| - |est[k, j, t, f]| | (k = 1..K-1;
 *   magnitudes float32 sqrtf(re^2 + im^2), float64 sums in a fixed order: bit-reproducible, as misonet_pit_select);
 *   L_k = the cheapest of the S! permutations (itertools.permutations order, first minimum: an all-silent overlap keeps
 *   the identity); P_0 = perm0_dev int32 [S] (NULL: identity), P_k[s] = L_k[P_{k-1}[s]].  perm_dev int32 [K, S] receives P
 *   (output speaker s of window k = est[k, P_k[s]]); perm0_dev may point at perm_dev's first row.  dist_dev: the first
 *   (K-1)*S*S doubles receive D_1..D_{K-1}, the rest is scratch; dist_bytes < misonet_css_scratch_bytes(K, S, F) returns
 *   MISONET_ENOMEM (dist_dev may be NULL when K == 1).  MISONET_EINVAL: S outside 1..4, F != 129, K < 1, hop_frames <= 0
 *   or fewer than 5 shared frames.
 *   A recording processed in batches carries the last window of a batch over as est[0] of the next, with its P as perm0.
 * misonet_css_stitch: y_dev float32 [K, S, W] = the iSTFT of the K windows (misonet_istft out_f32), perm_dev [K, S] = P.
 *   Sample m of the batch (k = min(K-1, m / H), j = m - kH) is y[k, P_k[s], j], for k >= 1 and j < ov cross-faded:
 *   c(j) y[k-1, P_{k-1}[s], H + j] + r(j) y[k, P_k[s], j], r(j) = sin^2, c(j) = cos^2 of pi (j + 1/2) / (2 ov), each
 *   evaluated in float64 and rounded to float32; int16 = the truncating cast of y * 32767 (as misonet_istft).
 *   first != 0: y[0] is window 0 of the recording and samples m = 0 .. n_out-1 are written; first == 0: y[0] is the window
 *   carried over from the previous call and samples m = H .. H + n_out - 1 (windows 1..K-1) are written.  out_i16_dev /
 *   out_f32_dev [S, n_out] (either may be NULL); n_out trims the padded tail on the last call.  MISONET_EINVAL: S outside
 *   1..4, K < 1, H outside [W/2, W - 256], n_out beyond the last window. */
long long misonet_css_scratch_bytes(int K, int S, int F);
int misonet_css_align(const void* est_dev, int K, int S, int T, int F, int hop_frames, const int* perm0_dev,
                      int* perm_dev, double* dist_dev, long long dist_bytes, misonet_stream stream);
int misonet_css_stitch(const float* y_dev, const int* perm_dev, int K, int S, int W, int hop, int first,
                       long long n_out, short* out_i16_dev, float* out_f32_dev, misonet_stream stream);

/* ---- scores of separated output against clean references (ABI 480) ------------------------------------------ */
/* misonet_score_wave: est_dev = E estimates per item, int16 (est_is_i16 != 0; a sample q stands for q / 32767) or float32;
 *   ref_dev = R references per item, float32.  Both are strided views: element (item b, source s, sample m) lies at
 *   base[b * sb + s * ss + m * st], strides in elements (int16 [B, S, n] from misonet_istft: (S n, n, 1); a time-major
 *   [B, n, S]: (n S, 1, S); one microphone c of [B, n, M], passed as base + c: (n M, 0, M) with E = 1).  Sample-contiguous
 *   views whose rows start 16-byte aligned are read with 16-byte loads.  n_valid_dev int32 [B] (NULL: n): samples
 *   [n_valid[b], n) of item b are left out (the zero-padded tail of a recording's last chunk).
 *   stats_dev double [B][E][R][5] receives (S e_i, S r_j, S e_i^2, S r_j^2, S e_i r_j) over the valid samples, accumulated
 *   in double (the int16 scale applied once, after the sums) in a fixed order without atomics: bit-reproducible, and the
 *   block of an item does not depend on B or on its position in the batch.  The statistics are additive over the chunks of
 *   a recording; SI-SDR, SNR and the best permutation follow from them on the host (misonet_amd/score.py).
 * misonet_score_spec: the reference's training criterion (criterion.py loss_uPIT / loss_Enhance) per pair of an
 *   estimate and a reference spectrogram: est_dev / ref_dev complex64 views, element (b, s, t, f) at base[b * sb + s * ss +
 *   t * st + f], strides in complex elements.  pair_dev double [B][E][R] = sum_{t,f} |Re e - Re r| + |Im e - Im r| +
 *   | sqrt(Re e^2 + Im e^2 + 1e-8) - |r| |, every term float32, summed in double in a fixed order.  perm_dev int32 [B][R]
 *   and upit_dev double [B] (either may be NULL; they need E == R): the permutation p with the least sum_i pair[i][p(i)]
 *   (itertools.permutations order, first minimum) and that sum.
 * scratch_dev: misonet_score_scratch_bytes(B, E, R, n) / (B, E, R, F) bytes = 8 B max(ceil(x / 4096) (2E + 2R + E R),
 *   min(x, 1024) E R); less returns MISONET_ENOMEM.  MISONET_EINVAL: a null argument, E outside 1..5, R outside 1..4,
 *   B outside 1..65535, n < 1, T < 1, F outside 1..1024, a negative stride.  Both calls are asynchronous on the stream,
 *   allocate nothing and can be captured into a HIP graph. */
long long misonet_score_scratch_bytes(int B, int E, int R, long long n_or_F);
int misonet_score_wave(const void* est_dev, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                       const float* ref_dev, long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R,
                       long long n, const int* n_valid_dev, double* stats_dev, void* scratch_dev,
                       long long scratch_bytes, misonet_stream stream);
int misonet_score_spec(const void* est_dev, long long est_sb, long long est_ss, long long est_st, const void* ref_dev,
                       long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R, int T, int F,
                       double* pair_dev, int* perm_dev, double* upit_dev, void* scratch_dev, long long scratch_bytes,
                       misonet_stream stream);

/* ---- BSS-eval SDR / SIR / SAR: the energies of the projections (ABI 490) ------------------------------------------ */
/* The metric of Vincent et al. 2006 (mir_eval.separation.bss_eval_sources): an estimate is projected onto the span of all
 * references delayed by 0 .. Q - 1 samples.  All arithmetic is float64; every signal is zero outside [0, n_valid).
 * misonet_bss_corr: the views, n_valid_dev and the int16 rule of misonet_score_wave.  Rrr_dev double [B][R][R][Q]:
 *   Rrr[j][k][a] = sum_t r_j[t] r_k[t + a]; Rre_dev double [B][R][E][Q]: Rre[j][i][a] = sum_t r_j[t] e_i[t + a]; Eee_dev
 *   double [B][E] = sum_t e_i[t]^2.  The products (exact in float64) are added over fixed 4096-sample segments on the
 *   float64 matrix pipe and the segments in segment order: bit-reproducible, independent of B and of the item's position.
 * misonet_bss_solve: G [R Q, R Q] with G[(j,a),(k,b)] = sum_t r_j[t - a] r_k[t - b] (block Toeplitz from Rrr), D_i = the
 *   Rre[.][i][.] stacked.  A_dev double [B][E] = D_i^T G^-1 D_i (the energy of the projection on all references), T_dev double
 *   [B][E][R] = d_ij^T G_jj^-1 d_ij (on reference j alone), by a blocked Cholesky factorisation whose forward substitution
 *   rides as extra rows.  A reference with Rrr[j][j][0] == 0 leaves the span (identity block, zero right-hand side: T = 0).
 *   info_dev int32 [B]: -1, or the first row of G whose pivot was <= 2^-40 of the matching diagonal entry of G or not finite;
 *   then every T and A of that item is NaN.  Eee_dev is not read by the kernels: SDR_ij = T / (Eee - T), SIR_ij = T / (A - T),
 *   SAR_i = A / (Eee - A) are formed on the host (misonet_amd/score.py).
 * scratch_dev: misonet_bss_scratch_bytes(B, E, R, n, Q) = 8 B max(ceil((n + 15) / 4096) (R R + R E + E) Q,
 *   (R Q + 4) R Q + R (Q + 4) Q) bytes (host only; misonet_bss_solve needs the value for n = 1); less returns MISONET_ENOMEM.
 *   MISONET_EINVAL (the size function: -1): a null argument, E or R outside 1..4, B outside 1..4096, Q outside 16..1024 or no
 *   multiple of 16, n outside 1..2^24, a negative stride.  Both calls are asynchronous on the stream and allocate nothing. */
long long misonet_bss_scratch_bytes(int B, int E, int R, long long n, int Q);
int misonet_bss_corr(const void* est_dev, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                     const float* ref_dev, long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R,
                     long long n, const int* n_valid_dev, int Q, double* Rrr_dev, double* Rre_dev, double* Eee_dev,
                     void* scratch_dev, long long scratch_bytes, misonet_stream stream);
int misonet_bss_solve(const double* Rrr_dev, const double* Rre_dev, const double* Eee_dev, int B, int E, int R, int Q,
                      double* T_dev, double* A_dev, int* info_dev, void* scratch_dev, long long scratch_bytes,
                      misonet_stream stream);

/* ---- STOI and ESTOI: the intelligibility figures (ABI 500) --------------------------------------------------------- */
/* STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of an estimate y against a clean reference x, step for step what
 * pystoi does (INTEGRATION.md 4f has the definition in full; tests/stoi_ref.py restates it): both signals resampled to
 * 10 kHz, the frames of 256 samples whose energy lies more than 40 dB under the loudest frame OF THE REFERENCE removed from
 * both, the kept frames overlap-added and framed again, a 512-point transform per frame, 15 third-octave bands from 150 Hz,
 * and over every run of 30 frames the clipped band-wise correlation (STOI) and the row- and column-normalised correlation
 * (ESTOI).  All arithmetic is float64, without atomics and in a fixed order: bit-reproducible, independent of B and of the
 * item's position in the batch.
 * misonet_stoi_resampled_len: ceil(n p / q) with p / q = 10000 / fs, the length at 10 kHz (host only); -1 for fs other than
 *   8000, 10000, 16000 or n outside 1..2^24.  misonet_stoi_taps: the number of polyphase taps 2 Lh + 1 (581 for 16 kHz, 365
 *   for 8 kHz, 1 for 10 kHz; host only), and, where taps_host is not NULL, the taps g[k] = p h[k - Lh] / sum h themselves.
 * misonet_stoi_resample: the views, n_valid_dev and the int16 rule of misonet_score_wave; mix_dev (may be NULL) float32, item
 *   b sample m at mix_dev[b * mix_sb + m * mix_st].  x10_dev double [B][R + E (+ 1)][n10], n10 = misonet_stoi_resampled_len(n,
 *   fs): the references, the estimates and the mixture at 10 kHz, x10[m] = sum_j x[j] g[m q - j p + Lh] with j ascending, zero
 *   past the item's own length; len10_dev int32 [B] = that length, ceil(n_valid p / q).  Every signal is resampled once.
 * misonet_stoi_measure: x10_dev as above (NS signals per item, the first R of them the references), len10_dev int32 [B] or
 *   NULL (n10).  out_dev double [B][NS - R][R][2] = (STOI, ESTOI) of estimate i against reference j, both 1e-5 where fewer
 *   than 30 frames are kept; frames_dev int32 [B][R][3] = (frames, kept frames, 1 if any sample of the reference is not
 *   zero).  The number of kept frames never leaves the device: the grids are sized by all frames.
 * scratch_dev: misonet_stoi_scratch_bytes(B, NS, R, n10) bytes (host only) = 8 B (R f + 15 R (NS - R + 1) f + 2 R (NS - R)
 *   max(f - 29, 1) + R ceil(f / 2)) with f = max(frames of n10, 1); less returns MISONET_ENOMEM.  MISONET_EINVAL (the size
 *   function: -1): a null argument, E or R outside 1..4, NS - R outside 1..5, B outside 1..4096, n outside 1..2^24, n10 outside
 *   1..5 * 2^22, another rate, a negative stride.  The first call on a device builds a table of 1715 doubles (window,
 *   twiddles, taps: one allocation and one synchronous copy); after that both calls are asynchronous on the stream and
 *   allocate nothing. */
long long misonet_stoi_resampled_len(long long n, int fs);
int misonet_stoi_taps(int fs, double* taps_host);
long long misonet_stoi_scratch_bytes(int B, int NS, int R, long long n10);
int misonet_stoi_resample(const void* est_dev, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                          const float* ref_dev, long long ref_sb, long long ref_ss, long long ref_st, const float* mix_dev,
                          long long mix_sb, long long mix_st, int B, int E, int R, long long n, const int* n_valid_dev, int fs,
                          double* x10_dev, int* len10_dev, misonet_stream stream);
int misonet_stoi_measure(const double* x10_dev, const int* len10_dev, int B, int NS, int R, long long n10, double* out_dev,
                         int* frames_dev, void* scratch_dev, long long scratch_bytes, misonet_stream stream);

/* ---- polyphase resampler: recordings at any sample rate (ABI 590) ------------------------------------------------------- */
/* scipy.signal.resample_poly's definition (= librosa's res_type="polyphase"; NOT librosa's default "soxr_hq", which was not
 * available and was not compared), restated (INTEGRATION.md 4o in full; tests/resample_ref.py restates it in NumPy).  With
 * p / q = fs_out / fs_in in lowest terms:
 *   Lh = 10 max(p, q);  h = firwin(2 Lh + 1, 1 / max(p, q), window = ("kaiser", 5.0));  g = p h
 *   y[m] = sum_j x[j] g[m q - j p + Lh],  j ascending over 0 <= j < n with the tap index inside [0, 2 Lh],  0 <= m < n_out
 *   n_out = ceil(n p / q);  zeros outside the signal (padtype "constant");  every channel on its own
 * p = q = 1 has Lh = 0 and g = {1}: an exact copy (or an exact conversion between the sample kinds below).  Admitted:
 * 1 <= max(p, q) <= 1024 (8 / 16 / 22.05 / 32 / 44.1 / 48 / 96 kHz against each other), 1 <= n <= 2^28 per channel, 1 <= M <= 16
 * channels, 1 <= B <= 65535 items; every index is 64-bit.  The taps are built on the host in float64 and kept on the device, one
 * table per (device, p, q), built at the first use there (one allocation and one synchronous copy); after that the call is
 * asynchronous on the stream, allocates nothing and can be captured in a HIP graph.  The sum is float64 in the order above and is
 * rounded once; no atomics: bit-reproducible, independent of B and of the item's position in the batch.  A non-finite input
 * sample reaches exactly the outputs whose support (tap index inside [0, 2 Lh]) contains it.
 * Sample kinds: 0 float32, 1 int16.  An int16 input sample q stands for q / 32767, scaled once after the sum (the int16 rule of
 * misonet_score_wave); an int16 output is the float64 result x 32767 rounded to nearest (ties to even) and saturated to
 * [-32768, 32767] (a NaN gives 0).  NOTE: the iSTFT's int16 store truncates toward zero, as the reference's astype(int16) does;
 * a resampler's output has no reference to follow and rounds.
 * Views: source element (item b, channel c, sample j) at src_dev[b * src_sb + c * src_sc + j * src_st], in elements of its kind;
 * the destination likewise with n_out samples.  Time-major [n][M] (a wav file) and channel-major [M][n] are both read with
 * coalesced loads; any other strides work.  n_valid_dev int32 [B] or NULL: item b's own length (clamped to [0, n]); its outputs
 * past ceil(n_valid p / q) are written as zeros, so every element of the destination view is written.
 * misonet_resample_ratio: p and q (either pointer may be NULL).  misonet_resampled_len: n_out.  misonet_resample_taps: the
 * number of taps 2 Lh + 1 and, where out_host is not NULL, g itself (cap = its capacity in doubles); host only, needs no GPU.
 * misonet_resample_tile: the output samples one workgroup owns (256), for tests that probe the tile edges.
 * MISONET_EINVAL (the size functions: -1), before any launch and before any pointer is looked at: a rate < 1, max(p, q) > 1024, n
 * outside 1..2^28, a kind other than 0 / 1, B or M outside their ranges, a negative source stride or src_st < 1, a destination
 * stride < 1 along an axis longer than 1, cap too small; then a null pointer. */
int misonet_resample_ratio(int fs_in, int fs_out, int* p, int* q);
long long misonet_resampled_len(long long n, int fs_in, int fs_out);
int misonet_resample_taps(int fs_in, int fs_out, double* out_host, int cap);
int misonet_resample_tile(void);
int misonet_resample(const void* src_dev, int src_kind, long long src_sb, long long src_sc, long long src_st, int B, int M,
                     long long n, const int* n_valid_dev, int fs_in, int fs_out, void* dst_dev, int dst_kind, long long dst_sb,
                     long long dst_sc, long long dst_st, misonet_stream stream);

/* ---- streaming polyphase resampler: waveform blocks in at one rate, blocks out at another (ABI 660) -----------------------
 * misonet_resample fed piece by piece, with its state on the device.  Ratio, taps, sum, sample kinds and
 * views are those above.  The bits do not depend on how a stream is cut into calls, and a stream that ends with `flush` has
 * emitted, concatenated, the result of misonet_resample of the whole signal BIT FOR BIT, for all four pairs of sample kinds.
 *
 * A stream has seen N = n_seen samples per channel.  Output m is complete once its last input floor((m q + Lh) / p) has arrived:
 * after N samples the stream has emitted e(N) outputs, e(N) = 0 where N p - 1 - Lh < 0 and floor((N p - 1 - Lh) / q) + 1
 * otherwise.  A call with n_new samples emits the outputs [e(N), E): E = e(N + n_new) without flush, E = ceil((N + n_new) p / q),
 * the offline length, with it (the last outputs skip the inputs past the end, as misonet_resample does).
 * misonet_resample_stream_outputs returns E - e(N); it may be 0, and the call still advances the state.  A stream flushed before
 * any sample emits nothing.
 *   src_dev    block of n_new samples, element (b, c, j) at src_dev[b * src_sb + c * src_sc + j * src_st] (NULL when n_new == 0)
 *   dst_dev    the call's outputs, output e(N) + i of (b, c) at dst_dev[b * dst_sb + c * dst_sc + i * dst_st], every one written
 *              (may be NULL when the call emits nothing)
 *   state_dev  misonet_resample_stream_state_bytes(B, M, fs_in, fs_out) bytes: float32 [B][M][C], the last
 *              C = misonet_resample_stream_carry(fs_in, fs_out) = floor(2 Lh / p) samples of the stream, aligned to its end, zero
 *              where the stream has not begun; an int16 sample is carried as its integer value.  No output needs more (the bound
 *              is tight): 60 samples for 48 -> 16 kHz, 20 for 16 -> 48 kHz, 55 for 44.1 -> 16 kHz, 20480 for 1 / 1024, 0 for
 *              1 / 1, where state_dev may be NULL and state_bytes 0.  misonet_resample_stream_reset writes every byte with zeros.
 *              After a flushing call the state is spent until the next reset.
 * The host passes n_seen: the kernels keep no counter on the device, and a launch depends on n_seen only through
 * e(N) q - N p, the place of the first output against the block's first sample in tap units, and through the counts.  Once
 * e(n_seen) > 0 a call whose n_new is a multiple of q can be captured into a HIP graph and replayed over the following blocks of
 * that length.  A call is one launch for the outputs (none when it emits nothing) and one small launch behind it that moves the
 * state on (none at a flush, none for 1 / 1); after the first use of a ratio on a device (its taps: one allocation, one synchronous
 * copy, not inside a capture) no host synchronisation and no allocation; no atomics; independent of B.
 * misonet_resample_stream_tile: the outputs one workgroup owns (32), for tests that probe the tile edges.
 * Latency: Lh / p input samples (30 samples, 0.625 ms, for 48 -> 16 kHz), plus the block.
 * Limits: 1 <= B <= 65535, 1 <= M <= 16, 0 <= n_new <= 2^28 (>= 1 unless flush), 0 <= n_seen <= 2^50, kinds 0 / 1, strides as
 * misonet_resample; anything else is MISONET_EINVAL (-1 from the size and count functions) before any launch and before any
 * pointer is looked at; then a null pointer; a short state is MISONET_ENOMEM. */
long long misonet_resample_stream_carry(long long fs_in, long long fs_out);                    /* C; -1 on a bad ratio */
long long misonet_resample_stream_state_bytes(int B, int M, long long fs_in, long long fs_out);
long long misonet_resample_stream_outputs(long long n_seen, long long n_new, int flush, long long fs_in, long long fs_out);  /* -1 on bad arguments */
int misonet_resample_stream_tile(void);
int misonet_resample_stream_reset(void* state_dev, int B, int M, long long fs_in, long long fs_out, misonet_stream stream);
int misonet_resample_stream(const void* src_dev, int src_i16, long long src_sb, long long src_sc, long long src_st, int B, int M,
                            long long n_new, long long n_seen, int flush, long long fs_in, long long fs_out, void* dst_dev,
                            int dst_i16, long long dst_sb, long long dst_sc, long long dst_st, void* state_dev,
                            long long state_bytes, misonet_stream stream);

/* ---- room simulator: image-source RIRs of a shoebox, and scene mixing (ABI 600) ------------------------------------------ */
/* The project's own definition in the Allen & Berkley (1979) family (INTEGRATION.md 4p in full; tests/room_ref.py restates it in
 * NumPy).  pyroomacoustics, gpuRIR, rir_generator and sms_wsj were not available: not compared against any of them.
 * misonet_room_rir.  All geometry as device pointers to doubles: room [B][3] the shoebox (Lx, Ly, Lz), one corner at the origin;
 * beta [B][6] the reflection coefficients in [0, 1) ordered x0, x1, y0, y1, z0, z1 ("0": the wall at coordinate 0, "1": at L);
 * src [B][S][3], mic [B][M][3].  With W = 80 and, per axis, N_i = ceil((Lh + W/2) c / (fs 2 L_i)): the images (n, q), n_i in
 * [-N_i, N_i], q_i in {0, 1}, enumerated n_x, n_y, n_z ascending, then q = q_x q_y q_z from 000 to 111 (q_z fastest);
 *   p_i = (1 - 2 q_i) s_i + 2 n_i L_i,  d = |p - r|,  tau = d fs / c,
 *   g = prod_i beta_i0^|n_i - q_i| beta_i1^|n_i| (0^0 = 1),  rho = sum_i (|n_i - q_i| + |n_i|);
 *   kept: g > 0 and (max_order < 0 or rho <= max_order);  a = g / (4 pi d);
 *   h[n] = sum over the kept images with |x| < W/2 of a 1/2 (1 + cos(2 pi x / W)) sinc(x),  x = n - tau,  0 <= n < Lh,
 * a float64 sum in the enumeration order; rir double [B][S][M][Lh].  fail int32 [B][S][M]: bit 0 a non-finite coordinate, a
 * point outside the room, a beta outside [0, 1) or an edge <= 0 (the RIR is all zero); bit 1 a kept image closer than 1e-3 m (a
 * source on a microphone), which is dropped; bit 2 more than 2^27 images or an N_i above 255 (the RIR is all zero).  max_order
 * -1: no limit.
 * misonet_room_mix.  src float32, element (b, s, j) at src_dev[b src_sb + s src_ss + j src_st]; rir double [B][S][M][Lh]; split
 * int32 [B][S] or NULL (= Lh);  images[b][s][m][n] = sum_{k = 0}^{min(n, Lh - 1)} h[k] x[n - k], x = 0 past L, k ascending, in
 * float64 FMAs, rounded once to float32, for 0 <= n < Lo; early the same sum over k < split[b][s]; mix[b][m][n] the float64 sum
 * of the unrounded image sums over s ascending, rounded once.  images float32 [B][S][M][Lo], early likewise or NULL, mix float32
 * [B][M][Lo] or NULL.
 * Both calls are asynchronous on the stream, allocate nothing, use no workspace (so MISONET_ENOMEM cannot arise) and can be
 * captured in a HIP graph; no atomics: bit-reproducible, independent of B and of the item's position in the batch; every
 * element of every output is written.  misonet_room_tile: the taps / output samples one workgroup owns (256), for tests that
 * probe the tile edges.  misonet_room_rir_len: B S M Lh; misonet_room_mix_len: the largest Lo, L + Lh - 1.
 * Limits: 1 <= B <= 4096, 1 <= S <= 4, 1 <= M <= 16, 1 <= Lh <= 2^16, 1 <= L <= 2^24, 1 <= Lo <= L + Lh - 1, B M Lo < 2^32.
 * MISONET_EINVAL (the size functions: -1) before any launch: outside these limits, fs or c not finite and > 0, max_order < -1,
 * a negative source stride or src_st < 1; then a null pointer. */
int misonet_room_tile(void);
long long misonet_room_rir_len(int B, int S, int M, int Lh);
long long misonet_room_mix_len(long long L, int Lh);
int misonet_room_rir(const double* room_dev, const double* beta_dev, const double* src_dev, const double* mic_dev, int B, int S,
                     int M, double fs, double c, int Lh, int max_order, double* rir_dev, int* fail_dev, misonet_stream stream);
int misonet_room_mix(const float* src_dev, long long src_sb, long long src_ss, long long src_st, const double* rir_dev,
                     const int* split_dev, int B, int S, int M, long long L, int Lh, long long Lo, float* images_dev,
                     float* early_dev, float* mix_dev, misonet_stream stream);

/* ---- source localisation: SRP, SRP-PHAT and MUSIC maps over a delay table, and their peaks (ABI 610) -------------------- */
/* The project's own definition in the SRP-PHAT / MUSIC family (DiBiase 2000; Schmidt 1986; INTEGRATION.md 4q in full,
 * tests/doa_ref.py restates it in NumPy float64).  pyroomacoustics was not available: nothing here was compared against it.
 * mix complex64 [B, F, M, T]; weight float32 [B, K, F, T] (the layout of the cACGMM masks) or NULL (K = 1, w = 1); tau float64
 * [Bg, D, M], the delay of candidate d at microphone m in seconds, Bg 1 or B, built on the host (far-field directions and
 * near-field points alike); pts float64 [D, 3], the candidates' coordinates, used only to keep peaks apart.  nfft = 2 (F - 1),
 * and 2 when F = 1; omega_f = 2 pi f fs / nfft.  Everything is float64 after the loads.
 * Blocks: block = 0 is one block over all T frames; otherwise hop = 0 means hop = block, N = 1 + (T - block) / hop in integer
 * division, block n covers the frames [n hop, n hop + block), the frames behind the last full block are not read.
 *   1. per (b, k, n, f), f_lo <= f <= f_hi:  R = sum_t w[b,k,f,t] x~_t x~_t^H over the block's frames, t ascending; kind
 *      srp_phat: x~_m = x_m / |x_m| and 0 where x_m = 0; otherwise x~ = x.  A bin that holds a non-finite sample, or a non-finite
 *      weight of class k, in that block is skipped and fail[b,k,n] |= 1; a bin with tr R = 0 is skipped.  srp, srp_phat:
 *      C_f = R.  music with S = num_src: the eigenpairs of R by the cyclic Jacobi of the beamformers, eigenvalues descending,
 *      equal ones lower index first; lambda_{S-1} <= 1e-12 lambda_0: the bin is skipped (its signal subspace has rank below S);
 *      otherwise C_f = (1 / M) sum_{r >= S} e_r e_r^H.  used[b,k,n] = the bins not skipped; used = 0: fail |= 2 and q = 0.
 *   2. per (b, k, n, d):  q = g sum_{f used, ascending} ( sum_m C_f[m,m] + 2 Re sum_{m<n} C_f[m,n] e^{+j omega_f (tau[d,m] - tau[d,n])} )
 *      = g sum_f a^H C_f a with a_m = e^{-j omega_f tau[d,m]};  g = 1 for srp and srp_phat (large at a source), g = 1 / used for
 *      music (q in [0, 1], small at a source).  q float64 [B, K, N, D].
 *   3. per (b, k, n), S rounds: the best candidate left -- the maximum of q, the minimum for music, ties to the lower index -- is
 *      taken; it and every candidate with |pts_d - pts_best|^2 < min_sep^2 are retired.  peak int32 [B, K, N, S], -1 once no
 *      candidate is left; value float64 [B, K, N, S], q at the peak, 0 beside a peak of -1.
 * Every sum has one fixed order and every output one writer: the results are bit-reproducible and the bits of a recording depend
 * neither on B nor on its position in the batch.  Three launches on the stream, no host synchronisation, no allocation: the call
 * can be captured in a HIP graph.  Every element of q, peak, value and fail is written.
 * Limits: 2 <= M <= 8, 1 <= K <= 8 (K = 1 without weights), 1 <= num_src <= min(4, D), music: num_src <= M - 1, 1 <= D <= 65536,
 * B, F, T >= 1, 0 <= f_lo <= f_hi < F (f_hi = -1, the default: F - 1), 0 <= block <= T, hop >= 0, min_sep finite and >= 0,
 * B K N D < 2^31, and the launch grids B N F < 2^26 and B K N ceil(D / tile) tile < 2^32, Bg 1 or B, fs finite and > 0; the
 * workspace 16-byte aligned.  Anything else is MISONET_EINVAL with a
 * message (misonet_doa_workspace_bytes and misonet_doa_blocks: -1) before any launch; then a null pointer; a short workspace is
 * MISONET_ENOMEM.  tau must be finite: the caller checks that on the host.
 * misonet_doa_tile: the candidates one workgroup of the steering kernel owns; misonet_doa_bin_chunk: the bins it stages at a
 * time; both for tests that probe the edges. */
typedef struct {
  int kind;                /* 0 "srp", 1 "srp_phat", 2 "music" */
  int num_src;             /* S: the peaks taken; for music also the dimension of the signal subspace */
  int block;               /* frames per block; 0 = all T */
  int hop;                 /* frames between blocks; 0 = block */
  int f_lo, f_hi;          /* the band, inclusive; f_hi -1 = F - 1 */
  double min_sep;          /* peaks are kept at least this far apart, in the unit of pts */
} misonet_doa_opts;
int misonet_doa_opts_default(misonet_doa_opts* opts);    /* 1, 1, 0, 0, 0, -1, 0.0 */
int misonet_doa_tile(void);
int misonet_doa_bin_chunk(void);
int misonet_doa_blocks(int T, int block, int hop);       /* N; -1 on bad arguments */
long long misonet_doa_workspace_bytes(int B, int K, int F, int M, int T, int D, const misonet_doa_opts* opts);
int misonet_doa(const void* mix_dev, const float* weight_dev_or_null, const double* tau_dev, int Bg, const double* pts_dev, int B,
                int K, int F, int M, int T, int D, double fs, const misonet_doa_opts* opts, double* q_out_dev, int* peak_out_dev,
                double* value_out_dev, int* fail_out_dev, void* ws_dev, long long ws_bytes, misonet_stream stream);
/* diagnostic: after misonet_doa with the same geometry and options, copy C complex128 [B, K, N, F, M, M] (0 for a bin that was
 * skipped or lies outside the band), used int32 [B, K, N] and fail int32 [B, K, N] to device buffers (any may be NULL) */
int misonet_doa_debug(const void* ws_dev, int B, int K, int F, int M, int T, int D, const misonet_doa_opts* opts,
                      void* c_c128_dev, int* used_dev, int* fail_dev, misonet_stream stream);

/* ---- online WPE: frame-recursive dereverberation, its state carried from call to call (ABI 620) -------------------------- */
/* The project's own definition in the RLS-WPE family (Yoshioka & Nakatani 2012; Caroselli et al. 2017; nara_wpe's online_wpe_step;
 * INTEGRATION.md 4r in full, tests/owpe_ref.py restates it in NumPy float64).  nara_wpe was not available: nothing here was compared
 * against it.  Audio is fed as it arrives: a call takes any T >= 1 new frames and advances the state; the memory does not grow.
 * Per (item b, bin f), independent of every other, N = M taps.  State: P complex128 [N, N], G complex128 [N, M], the last
 * delay + taps - 1 observed frames (the complex64 that was read), the mean-over-microphones powers of the last `context` frames,
 * n (the frames seen) and the fail word.  misonet_owpe_reset: P = init I, everything else 0.  Per new frame y, float64 after the load:
 *   1. z[k M + m] = y[m, t - delay - k]   (k = 0 .. taps - 1; the row order of misonet_wpe; 0 before the start of the stream)
 *   2. x = y - G^H z                      the output, rounded to complex64 once
 *   3. lambda = max(mean of p over the min(n, context) + 1 most recent frames, this one included, power_floor), p = mean_m |y_m|^2
 *      (the floor is absolute: one relative to max_t p would not be causal)
 *   4. u = P z;  d = alpha lambda + Re(z^H u);  k = u / d
 *   5. P <- (P - k u^H) / alpha           the lower triangle is computed and mirrored: P stays exactly Hermitian
 *   6. G <- G + k x^H
 *   7. the frame enters the frame ring, p the power ring, n <- n + 1 (n stops at 2^31 - 1)
 * A failing frame -- a non-finite sample in it, or d not finite or not > 0 -- is passed through: x = y, P and G stay, the frame
 * enters the frame ring as zeros and p as 0, fail[b, f] |= 1, n advances.  Nothing is clamped.  (Silence with alpha < 1 multiplies
 * P by 1 / alpha per frame; reset the stream before that overflows, after 7e5 frames at alpha 0.999.)
 * Every sum runs in one fixed order, without atomics: the bits of an item depend neither on B, nor on its position in the batch,
 * nor on how the stream is cut into calls.  misonet_owpe is one launch, with no host synchronisation and no allocation: it can be
 * captured in a HIP graph (after one misonet_owpe_reset on that device outside the capture).
 * mix_dev and out_dev are complex64 [B, M, T, F]; they must not be the same buffer.  state_dev: misonet_owpe_state_bytes bytes,
 * 16-byte aligned, written by misonet_owpe_reset before the first call; its size does not depend on T.  1 <= M <= 8,
 * M taps <= 80, delay >= 1 (and small enough for the frame ring to fit the 160 KB of LDS beside P: misonet_owpe_lds_bytes),
 * 0 <= context <= 16, 0 < alpha <= 1, power_floor and init finite and > 0, B F < 2^31: anything else is refused on the host with
 * MISONET_EINVAL and a message (the size functions: -1), before any launch; a short state is MISONET_ENOMEM. */
typedef struct {
  int taps;
  int delay;
  int context;             /* earlier frames in the power estimate */
  double alpha;            /* forgetting factor */
  double power_floor;      /* absolute */
  double init;             /* P = init I at reset */
} misonet_owpe_opts;
int misonet_owpe_opts_default(misonet_owpe_opts* opts);  /* 10, 3, 0, 0.999, 1e-10, 1.0 */
long long misonet_owpe_state_bytes(int B, int M, int F, const misonet_owpe_opts* opts);
int misonet_owpe_lds_bytes(int M, const misonet_owpe_opts* opts);   /* the LDS one workgroup takes; -1 on bad arguments */
int misonet_owpe_reset(void* state_dev, int B, int M, int F, const misonet_owpe_opts* opts, misonet_stream stream);
int misonet_owpe(const void* mix_dev, int B, int M, int T, int F, const misonet_owpe_opts* opts, void* out_dev, void* state_dev,
                 long long state_bytes, misonet_stream stream);
/* diagnostic: copy G complex128 [B, F, M taps, M], P complex128 [B, F, M taps, M taps], fail int32 [B, F] and n int32 [B, F] out
 * of the state to device buffers (any may be NULL) */
int misonet_owpe_debug(const void* state_dev, int B, int M, int F, const misonet_owpe_opts* opts, void* g_c128_dev,
                       void* p_c128_dev, int* fail_dev, int* n_dev, misonet_stream stream);

/* ---- online AuxIVA: frame-recursive blind separation, its state carried from call to call (ABI 630) ---------------------- */
/* The project's own definition in the online-AuxIVA family (Taniguchi, Ono, Kawamura & Sagayama 2014; INTEGRATION.md 4s in full,
 * tests/oiva_ref.py restates it in NumPy float64).  pyroomacoustics and torchiva were not available: nothing here was compared
 * against them.  Audio is fed as it arrives: a call takes any T >= 1 new frames and advances the state; the memory does not grow.
 * Each item b runs on its own.  The determined case only: K = M sources, no PCA, 2 <= M <= 8.
 * State per (b, f): W complex128 [M, M] (row k is w_k^H, y = W x), V complex128 [M, M, M] (one Hermitian M x M matrix per
 * source), n int32 (the frames seen; it stops at 2^31 - 1) and fail int32.  misonet_oiva_reset: W = I, V_k = init I, n = 0,
 * fail = 0; it writes every byte of the state.  Per new frame, x_f the frame's M samples of bin f, float64 after the load:
 *   0. a bin whose frame holds a non-finite sample: fail |= 1; its x_f counts as 0 in steps 1-2, step 3 is skipped for it (W
 *      and V stay) and its outputs for this frame are 0
 *   1. yt_k[f] = sum_m W_f[k, m] x_f[m], m ascending, with W as it stood before this frame
 *   2. r_k = sum_f |yt_k[f]|^2, in one fixed order that depends on M and F alone (not on B, T or the cut);
 *      model 0 "gauss": phi_k = 1 / max(r_k / F, floor);  model 1 "laplace": phi_k = 1 / max(2 sqrt(r_k), floor)
 *      (the formulas of misonet_auxiva with one frame in the place of all)
 *   3. per bin, for k = 0 .. M - 1 in order:
 *        V_k <- alpha V_k + (1 - alpha) phi_k x x^H   the lower triangle is computed and mirrored, the diagonal's imaginary part
 *                                                     is exactly 0: V_k stays exactly Hermitian
 *        (W V_k) u = e_k                              W with the rows already replaced in this frame.  Gaussian elimination with
 *                                                     partial pivoting and back substitution; the pivot is the largest
 *                                                     |re| + |im| of the column (a non-finite one counts as the largest), ties
 *                                                     go to the lower row
 *        d = Re(u^H V_k u)
 *        a pivot 0 or non-finite, or d not finite or not > 0: row k stays and fail |= 2; otherwise row k of W <- conj(u) / sqrt(d)
 *   4. y = W x with the new W;  A = W^-1 by the same elimination (one column per e_j);  est[k] = A[ref_ch, k] y_k,
 *      images[k, m] = A[m, k] y_k, each rounded once to complex64;  W singular: fail |= 4 and the outputs of this (f, t) are 0
 *   5. n <- n + 1
 * Nothing is clamped.  Every sum runs in one fixed order, without atomics: the bits of an item depend neither on B, nor on its
 * position in the batch, nor on how the stream is cut into calls.  misonet_oiva is one launch for any T >= 1, with no host
 * synchronisation and no allocation: it can be captured in a HIP graph (after one misonet_oiva_reset outside the capture).
 * Every element of every output is written.
 * mix_dev complex64 [B, M, T, F]; est_out_dev complex64 [B, M(k), T, F]; images_out_dev (may be NULL) complex64
 * [B, M(k), M, T, F]; no two of them may overlap.  state_dev: misonet_oiva_state_bytes bytes, 16-byte aligned, written by
 * misonet_oiva_reset before the first call; its size does not depend on T.  2 <= M <= 8, B >= 1, T >= 1, 1 <= F <= 1025,
 * 0 < alpha < 1 (1 would freeze V), floor and init finite and > 0, 0 <= ref_ch < M, B F < 2^31: anything else is refused on the
 * host with MISONET_EINVAL and a message (the size functions: -1), before any launch and before any pointer is looked at; a
 * short state is MISONET_ENOMEM.  misonet_oiva_bins_per_pass: the bins of an item that one workgroup covers at once (for tests
 * that probe the edges). */
typedef struct {
  int model;               /* 0 gauss, 1 laplace */
  int ref_ch;              /* the microphone est is projected to */
  double alpha;            /* forgetting factor */
  double floor;            /* under the weights' denominators, absolute */
  double init;             /* V_k = init I at reset */
} misonet_oiva_opts;
int misonet_oiva_opts_default(misonet_oiva_opts* opts);  /* 0, 0, 0.98, 1e-10, 1.0 */
long long misonet_oiva_state_bytes(int B, int M, int F);
int misonet_oiva_bins_per_pass(int M);
int misonet_oiva_reset(void* state_dev, int B, int M, int F, const misonet_oiva_opts* opts, misonet_stream stream);
int misonet_oiva(const void* mix_dev, int B, int M, int T, int F, const misonet_oiva_opts* opts, void* est_out_dev,
                 void* images_out_dev_or_null, void* state_dev, long long state_bytes, misonet_stream stream);
/* diagnostic: copy W complex128 [B, F, M, M], V complex128 [B, F, M, M, M], fail int32 [B, F] and n int32 [B, F] out of the state
 * to device buffers (any may be NULL) */
int misonet_oiva_debug(const void* state_dev, int B, int M, int F, void* w_c128_dev, void* v_c128_dev, int* fail_dev, int* n_dev,
                       misonet_stream stream);

/* ---- online AuxIVA for fewer sources than microphones: K rows out, its state carried from call to call (ABI 670) --------- */
/* The project's own definition in the OverIVA family (Scheibler & Ono, "Independent vector analysis with more microphones than
 * sources", WASPAA 2019) in the frame-recursive form of misonet_oiva (INTEGRATION.md 4w in full, tests/overiva_ref.py restates it
 * in NumPy float64).  pyroomacoustics and torchiva were not available: nothing here was compared against them.  Audio is fed as
 * it arrives: a call takes any T >= 1 new frames and advances the state; the memory does not grow.  Each item b runs on its own.
 * K sources at M microphones, 2 <= M <= 8 and 1 <= K <= M - 1; K = 1 is blind extraction of one source; K = M is refused with a
 * message that names misonet_oiva.  The options are misonet_oiva_opts: K is a dimension, not an option.
 * State per (b, f), all complex128: Ws [K, M] (row k is w_k^H, y = Ws x), J [M - K, K], V [K, M, M] (one Hermitian matrix per
 * source), C [M, M] (Hermitian, the recursive mixture covariance); n int32 (the frames seen; it stops at 2^31 - 1) and fail
 * int32.  The full demixing matrix is W = [Ws ; J, -I_{M-K}].  misonet_overiva_reset: Ws = [I_K 0], J = 0, V_k = init I,
 * C = init I, n = 0, fail = 0; it writes every byte of the state.  Per new frame, x the frame's M samples of bin f, float64
 * after the load:
 *   0. a bin whose frame holds a non-finite sample: fail |= 1; its x counts as 0 in steps 1-2, step 3 is skipped for it (Ws, J, V
 *      and C stay) and its outputs for this frame are 0
 *   1. yt_k[f] = sum_m Ws_f[k, m] x_f[m], m ascending, for k < K, with Ws as it stood before this frame
 *   2. r_k = sum_f |yt_k[f]|^2, in one fixed order that depends on M, K and F alone;
 *      model 0 "gauss": phi_k = 1 / max(r_k / F, floor);  model 1 "laplace": phi_k = 1 / max(2 sqrt(r_k), floor)
 *   3. per bin:  C <- alpha C + (1 - alpha) x x^H     the lower triangle is computed, the upper is its mirror, the diagonal's
 *                                                     imaginary part is exactly 0
 *      then, for k = 0 .. K - 1 in order:
 *        V_k <- alpha V_k + (1 - alpha) phi_k x x^H   by the same rule: C and every V_k stay exactly Hermitian
 *        (W V_k) u = e_k                              the full M x M W as it stands, with the rows replaced and the J re-solved
 *                                                     earlier in this frame; the elimination of misonet_oiva: partial pivoting
 *                                                     on |re| + |im|, a non-finite entry counts as the largest, ties go to the
 *                                                     lower row, then back substitution
 *        d = Re(u^H V_k u)
 *        a pivot 0 or non-finite, or d not finite or not > 0: row k stays and fail |= 2; otherwise row k of Ws <- conj(u) / sqrt(d)
 *        J is re-solved after every k, not once per frame: P = C Ws^H [M, K], summed over m ascending, P1 its first K rows and
 *        P2 its last M - K; J P1 = P2 is solved as P1^T J^T = P2^T by the same elimination (K x K, M - K right-hand sides);
 *        a pivot 0 or non-finite: J stays and fail |= 8
 *   4. y_k = sum_m Ws[k, m] x[m] with the new Ws;  S = Ws[:, :K] + Ws[:, K:] J (K x K);  A_top = S^-1 by the same elimination with
 *      right-hand side I_K;  A_bot = J A_top;  A = [A_top; A_bot] is the first K columns of W^-1;  est[k] = A[ref_ch, k] y_k,
 *      images[k, m] = A[m, k] y_k, each rounded once to complex64;  S singular: fail |= 4 and the outputs of this (f, t) are 0
 *   5. n <- n + 1
 * Nothing is clamped.  By construction [J, -I] C Ws^H = 0 after step 3, Re(w_k^H V_k w_k) = 1 and W A = [I_K; 0].  sum_k images = x
 * does NOT hold as it does for misonet_oiva: the background is what is left.  Every sum runs in one fixed order, without
 * atomics: the bits of an item depend neither on B, nor on its position in the batch, nor on how the stream is cut into calls.
 * misonet_overiva is one launch for any T >= 1, with no host synchronisation and no allocation: it can be captured in a HIP
 * graph (after one misonet_overiva_reset outside the capture).  Every element of every output is written.
 * mix_dev complex64 [B, M, T, F]; est_out_dev complex64 [B, K, T, F]; images_out_dev (may be NULL) complex64 [B, K, M, T, F]; no
 * two of them may overlap.  state_dev: misonet_overiva_state_bytes bytes, 16-byte aligned, written by misonet_overiva_reset
 * before the first call; its size does not depend on T.  2 <= M <= 8, 1 <= K <= M - 1, B >= 1, T >= 1, 1 <= F <= 1025, the
 * fields of opts as misonet_oiva takes them (0 <= ref_ch < M), B F < 2^31: anything else is refused on the host with
 * MISONET_EINVAL and a message (the size functions: -1), before any launch and before any pointer is looked at; a short state
 * is MISONET_ENOMEM.  misonet_overiva_bins_per_pass: the bins of an item that one workgroup covers at once. */
long long misonet_overiva_state_bytes(int B, int M, int K, int F);
int misonet_overiva_bins_per_pass(int M, int K);
int misonet_overiva_reset(void* state_dev, int B, int M, int K, int F, const misonet_oiva_opts* opts, misonet_stream stream);
int misonet_overiva(const void* mix_dev, int B, int M, int K, int T, int F, const misonet_oiva_opts* opts, void* est_out_dev,
                    void* images_out_dev_or_null, void* state_dev, long long state_bytes, misonet_stream stream);
/* diagnostic: copy Ws complex128 [B, F, K, M], J complex128 [B, F, M - K, K], V complex128 [B, F, K, M, M], C complex128
 * [B, F, M, M], fail int32 [B, F] and n int32 [B, F] out of the state to device buffers (any may be NULL) */
int misonet_overiva_debug(const void* state_dev, int B, int M, int K, int F, void* ws_c128_dev, void* j_c128_dev, void* v_c128_dev,
                          void* c_c128_dev, int* fail_dev, int* n_dev, misonet_stream stream);

/* ---- online beamformer: frame-recursive MVDR / MWF, its state carried from call to call (ABI 640) ------------------------ */
/* The project's own definition in the family of mask- or estimate-driven beamformers with exponentially forgotten spatial
 * covariance matrices, re-solved every frame (Souden, Benesty & Affes 2010 for the filter; Higuchi et al. 2017 and Boeddeker et
 * al. 2018 for the recursive use; INTEGRATION.md 4t in full, tests/obf_ref.py restates it in NumPy float64).  pb_bss, ESPnet,
 * nara_wpe and pyroomacoustics were not available: nothing here was compared against them.  Audio is fed as it arrives: a call
 * takes any T >= 1 new frames and advances the state; the memory does not grow.  Every cell (item b, source s, bin f) runs on
 * its own: nothing couples bins, sources or items.
 * State per cell: Phi_s and Phi_n complex128 [M, M], Hermitian; w complex128 [M], the filter of the last frame (stored for
 * misonet_obf_debug, never read by the recursion); n int32 (the frames seen; it stops at 2^31 - 1) and fail int32.
 * misonet_obf_reset: Phi_s = 0, Phi_n = init I, w = 0, n = 0, fail = 0; it writes every byte of the state.  Per new frame t, y the
 * M samples of mix and x the M samples of images[b, s], float64 after the loads:
 *   0. a non-finite sample in y or x: fail |= 1; Phi_s, Phi_n and w stay, out = 0 for this frame; step 7 still runs
 *   1. v = y - x for noise 0 "residual"; v = y for noise 1 "mix" (MPDR)
 *   2. Phi_s <- alpha Phi_s + (1 - alpha) x x^H, Phi_n <- alpha Phi_n + (1 - alpha) v v^H: the lower triangle is computed and
 *      mirrored, the diagonal's imaginary part is exactly 0: the stored matrices are exactly Hermitian
 *   3. R = Phi_n + (diag_load tr(Phi_n) / M + epsi) I, tr the sum of the real diagonal with m ascending
 *   4. R = L L^H without pivoting, column by column, the inner sums over k ascending; 1 / L[c][c] is formed once and multiplies
 *      wherever L[c][c] divides.  A pivot not finite or not > 0: fail |= 2, w = 0 and out = 0 for this frame (step 2 stays)
 *   5. G = R^-1 Phi_s by the two triangular solves (forward with k ascending, backward with k descending);
 *      den = mu + sum_m G[m, m], m ascending (the complex trace).  den not finite: fail |= 4, w = 0, out = 0.  den exactly 0 (a
 *      source silent so far): w = 0, out = 0, no flag.  Otherwise w = G[:, ref_ch] (1 / den), the reciprocal in Smith's form.
 *      mu = 0 is the Souden MVDR, mu > 0 the rank-1 / speech-distortion-weighted MWF
 *   6. out = sum_m conj(w_m) y_m, m ascending, rounded once to complex64
 *   7. n <- n + 1
 * Nothing is clamped.  The filter of frame t uses frame t's own sample and no later one: causal, no look-ahead.  Every sum runs in
 * one fixed order that depends on M alone, without atomics: the bits of a cell depend neither on B, nor on its position in the
 * batch, nor on how the stream is cut into calls.  misonet_obf is one launch for any T >= 1, with no host synchronisation and no
 * allocation: it can be captured in a HIP graph (after one misonet_obf_reset outside the capture).  Every element of out is
 * written.
 * mix_dev complex64 [B, M, T, F]; images_dev complex64 [B, S, M, T, F]; out_dev complex64 [B, S, T, F]; none of them and the state
 * may overlap.  state_dev: misonet_obf_state_bytes bytes, 16-byte aligned, written by misonet_obf_reset before the first call;
 * its size does not depend on T.  2 <= M <= 8, 1 <= S <= 8, B >= 1, T >= 1, 1 <= F <= 1025, B S F < 2^31, noise 0 or 1,
 * 0 <= ref_ch < M, 0 < alpha < 1 (1 would freeze Phi), mu, diag_load, epsi and init finite and >= 0: anything else is refused on
 * the host with MISONET_EINVAL and a message (the size functions: -1), before any launch and before any pointer is looked at; a
 * short state is MISONET_ENOMEM.  misonet_obf_cells_per_block: the cells one workgroup covers (for tests that probe the edges). */
typedef struct {
  int noise;               /* 0 residual (v = y - x), 1 mix (v = y) */
  int ref_ch;              /* the reference microphone */
  double alpha;            /* forgetting factor */
  double mu;               /* 0: Souden MVDR; > 0: rank-1 / SDW multichannel Wiener filter */
  double diag_load;        /* R = Phi_n + (diag_load tr(Phi_n) / M + epsi) I */
  double epsi;
  double init;             /* Phi_n = init I at reset */
} misonet_obf_opts;
int misonet_obf_opts_default(misonet_obf_opts* opts);  /* 0, 0, 0.98, 0.0, 1e-3, 1e-10, 1.0 */
long long misonet_obf_state_bytes(int B, int S, int M, int F);
int misonet_obf_cells_per_block(int M);
int misonet_obf_reset(void* state_dev, int B, int S, int M, int F, const misonet_obf_opts* opts, misonet_stream stream);
int misonet_obf(const void* mix_dev, const void* images_dev, int B, int S, int M, int T, int F, const misonet_obf_opts* opts,
                void* out_dev, void* state_dev, long long state_bytes, misonet_stream stream);
/* diagnostic: copy Phi_s and Phi_n complex128 [B, S, F, M, M], w complex128 [B, S, F, M], fail int32 [B, S, F] and n int32
 * [B, S, F] out of the state to device buffers (any may be NULL) */
int misonet_obf_debug(const void* state_dev, int B, int S, int M, int F, void* phi_s_c128_dev, void* phi_n_c128_dev,
                      void* w_c128_dev, int* fail_dev, int* n_dev, misonet_stream stream);

/* ---- cepstral distance, LLR, fwSegSNR: the dereverberation figures (ABI 540) ------------------------------------------- */
/* The three measures the REVERB challenge judges dereverberation by, of an estimate y against a clean reference x, as
 * INTEGRATION.md 4j defines them in full (tests/reverb_ref.py restates it; the challenge's MATLAB tools were not available, so
 * the figures have not been compared against them): frames of N = fs / 40 samples (25 ms) every H = fs / 100 (10 ms) under
 * MATLAB's hanning(N), a transform of NFFT = 256 (8 kHz) or 512 (16 kHz) points, and per frame of every signal 25 real cepstral
 * coefficients (floor 1e-15 on the magnitudes), 23 mel band sums of the magnitudes, the autocorrelation at lags 0..12 and the
 * LPC of order 12 by Levinson-Durbin.  Per pair: the frames whose reference has r[0] > 0 are used (K of them); CD is the
 * mean-normalised cepstral distance in dB capped at 10, LLR = ln(a_y' R_x a_y / a_x' R_x a_x) clipped to [0, 2] over the
 * K_llr used frames where neither recursion failed and both forms are positive, fwSegSNR the mean over the bands, weighted by
 * (g_x X_b)^0.2, of 10 log10(X_b^2 / (X_b - Y_b)^2) clipped to [-10, 35] after both signals are scaled to unit power.  All
 * arithmetic after the loads is float64, without floating-point atomics and in a fixed order: bit-reproducible, independent of
 * B, of the item's position in the batch and of the layout; samples past n_valid are not read.
 * misonet_reverb_frames: the frames of n samples, (n - N) / H + 1 or 0 for n < N (host only); -1 for fs other than 8000, 16000
 *   or n outside 1..2^24.
 * misonet_reverb_measure: the views, n_valid_dev and the int16 rule of misonet_score_wave; mix_dev (may be NULL) as in
 *   misonet_stoi_resample: the mixture is measured as one more estimate, the last.  out_dev double [B][E (+ 1)][R][6] = (CD
 *   mean, CD median, LLR mean, LLR median, fwSegSNR mean, fwSegSNR median) over the counted frames of estimate i against
 *   reference j, all NaN where K = 0 or the reference is silent, the LLR pair NaN where K_llr = 0; the median of an even count
 *   is the mean of the two middle values.  count_dev int32 [B][E (+ 1)][R][3] = (frames of n_valid, K, K_llr).  frame_dev (may
 *   be NULL) double [B][E (+ 1)][R][3][misonet_reverb_frames(n, fs)]: the CD, LLR and fwSegSNR of every frame, NaN where the
 *   frame is not counted; entries past the frames of the item's n_valid are not written.
 * scratch_dev: misonet_reverb_scratch_bytes(B, NS, R, n, fs) bytes (host only), NS = R + E (+ 1) = the signals of an item, =
 *   8 B (NS + 75 NS f + 3 (NS - R) R f) with f = max(frames of n, 1); less returns MISONET_ENOMEM.  MISONET_EINVAL (the size
 *   functions: -1): a null argument, E or R outside 1..4, NS - R outside 1..5, B outside 1..4096, n outside 1..2^24, another
 *   rate, a negative stride.  The first call on a device builds a table of 10082 doubles (twiddles, windows, mel triangles:
 *   one allocation and one synchronous copy); after that the call is asynchronous on the stream and allocates nothing. */
long long misonet_reverb_frames(long long n, int fs);
long long misonet_reverb_scratch_bytes(int B, int NS, int R, long long n, int fs);
int misonet_reverb_measure(const void* est_dev, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                           const float* ref_dev, long long ref_sb, long long ref_ss, long long ref_st, const float* mix_dev,
                           long long mix_sb, long long mix_st, int B, int E, int R, long long n, const int* n_valid_dev, int fs,
                           double* out_dev, int* count_dev, double* frame_dev, void* scratch_dev, long long scratch_bytes,
                           misonet_stream stream);

/* ---- SRMR: the figure that needs no clean reference (ABI 550) ------------------------------------------------------------- */
/* The speech-to-reverberation modulation energy ratio (Falk, Zheng & Chan 2010) of a signal, as INTEGRATION.md 4k defines it in
 * full (tests/srmr_ref.py restates it; no SRMR toolbox was available, so the figure has not been compared against one): a
 * 23-channel gammatone bank (Slaney's ERB filters, 125 Hz .. fs / 2), per channel the magnitude of the analytic signal over the
 * whole recording (a transform of P = the smallest power of two >= n points), eight second-order modulation filters (4 .. 128 Hz,
 * Q = 2) at the full rate, the energy of every 256 ms frame (64 ms hop, symmetric Hamming window) averaged over the frames, and
 * the ratio of the energy in the four lowest modulation bands to that in bands 4 .. K* - 1, K* in 5..8 following the bandwidth
 * of the channel that completes 90 % of the energy from the top.  All arithmetic after the loads is float64, without
 * floating-point atomics and in a fixed order: bit-reproducible, independent of B, of the item's position in the batch and of the
 * layout; samples past n_valid are not read, and P, the chunks and the frames of an item follow its own n_valid.
 * misonet_srmr_frames: the frames of n samples, 1 + (n - N_w) / H_w or 0 for n < N_w, N_w = ceil(0.256 fs), H_w = ceil(0.064 fs)
 *   (host only); -1 for fs other than 8000, 16000 or n outside 0..2^24.
 * misonet_srmr_chunk: the samples C of a chunk of the scan that runs the recurrences in parallel along time (host only).
 * misonet_srmr_measure: sig_dev, its strides, n_valid_dev and the int16 rule as the estimates of misonet_score_wave, S signals
 *   per item; mix_dev (may be NULL) as in misonet_stoi_resample: the mixture is measured as one more signal, the last.  out_dev
 *   double [B][S (+ 1)][3] = (SRMR, K*, BW in Hz); (NaN, 0, NaN) for a signal shorter than one frame or without energy.
 *   count_dev int32 [B][S (+ 1)] = the frames of n_valid.  energy_dev (may be NULL) double [B][S (+ 1)][23][8]: the mean
 *   modulation energies, channels ascending; NaN for a signal shorter than one frame.
 * scratch_dev: misonet_srmr_scratch_bytes(B, NS, n, fs) bytes (host only), NS = S (+ 1): the 184 means of every signal and as
 *   many slots of one (signal, channel) as fit 1 GiB (at least one; a slot is 8 (n + 2 P [P > 4096] + 24 chunks + 32 hops)
 *   bytes), so the size is bounded whatever B; less returns MISONET_ENOMEM.  MISONET_EINVAL (the size functions: -1): a null
 *   argument, S outside 1..4, NS outside 1..5, B outside 1..4096, n outside 1..2^24, another rate, a negative stride.  The first
 *   call on a device builds a table of 28080 doubles (twiddles, windows, coefficients, transitions: one allocation and one
 *   synchronous copy); after that the call is asynchronous on the stream, allocates nothing and can be captured. */
long long misonet_srmr_frames(long long n, int fs);
long long misonet_srmr_scratch_bytes(int B, int NS, long long n, int fs);
int misonet_srmr_chunk(void);
int misonet_srmr_measure(const void* sig_dev, int sig_is_i16, long long sig_sb, long long sig_ss, long long sig_st,
                         const float* mix_dev, long long mix_sb, long long mix_st, int B, int S, long long n,
                         const int* n_valid_dev, int fs, double* out_dev, int* count_dev, double* energy_dev, void* scratch_dev,
                         long long scratch_bytes, misonet_stream stream);

/* ---- fused on-device pipeline: the body of Tester_Enhance.inference (tester.py:865-939) -------------------- */
/* MISO1_Inference (6 circular shifts batched as 6B forwards, tester.py:1014-1068) -> clean-reference
 * alignment (tester.py:889-915; skipped when clean_dev == NULL) -> MVDR per speaker (tester.py:917-924) ->
 * MISO3 per speaker (tester.py:936-939).  Everything stays in HBM in the kernels' own layout. */
/* 2 <= num_mic <= 8; 1 <= num_spk <= 4 (the reference's own clean-reference alignment stacks exactly s0 and s1,
 * tester.py:889-891, i.e. its harness is 2-speaker; here clean_dev simply carries num_spk sources).
 * miso3 == NULL creates a SEPARATION-ONLY pipeline (the body the reference's Tester_Beamforming shares with
 * Tester_Enhance, tester.py:340-449: MISO1_Inference + alignments, no MISO3 memory): misonet_pipeline_run then needs
 * out_dev == NULL and bf_dev == NULL (MISONET_ESTATE otherwise). */
int misonet_pipeline_create(misonet_net* miso1, misonet_net* miso3, int num_mic, int num_spk, int ref_ch,
                            float epsi, misonet_pipeline** out);
int misonet_pipeline_destroy(misonet_pipeline* p);
/* ABI 510: the beamformer of step "MVDR per speaker" (misonet_pipeline_create sets the defaults with its own epsi and
 * ref_ch 0).  Legal between runs; the workspace size depends on the kind, so misonet_pipeline_workspace_bytes must be asked
 * again.  MISONET_EINVAL for bad fields (as misonet_beamform, M = num_mic).  The options are kernel arguments: a HIP graph
 * captured from a run keeps the options it was captured with, and the library holds no graph itself, so no call order can
 * make this return MISONET_ESTATE; the owner of a captured graph captures again (misonet_amd.Enhancer refuses the change
 * while one of its captured passes is alive). */
int misonet_pipeline_set_beamformer(misonet_pipeline* p, const misonet_bf_opts* opts);
/* ABI 530: WPD as that step, per aligned speaker, on the same views and into the same beamformer planes (M = num_mic; the source
 * estimate is MISO1's at every microphone).  opts == NULL: back to the misonet_bf_opts that are set.  Legal between runs; the
 * workspace size depends on it (ask misonet_pipeline_workspace_bytes again); a run with T <= delay + taps - 1 frames is refused
 * with MISONET_EINVAL.  MISONET_EINVAL for bad fields (as misonet_wpd).  With WPD not set every bit of every path is unchanged. */
int misonet_pipeline_set_wpd(misonet_pipeline* p, const misonet_wpd_opts* opts);
/* ABI 560: a step between the alignments and the beamformer: initial masks from the aligned MISO1 estimates and the mixture
 * (misonet_masks_from_estimates), misonet_cacgmm with these options, and the refined images gamma_s Y as the source estimate of
 * whichever beamformer is set.  MISO3's third input and miso1_dev stay the raw MISO1 estimate.  opts == NULL: off again.  Legal
 * between runs; the workspace grows only while it is set (ask misonet_pipeline_workspace_bytes again).  MISONET_EINVAL for bad
 * fields (as misonet_cacgmm).  With it not set every bit of every path and the workspace size are unchanged. */
int misonet_pipeline_set_refine(misonet_pipeline* p, const misonet_cacgmm_opts* opts);
/* ABI 570: a joint beamformer (misonet_beamform_joint) as step 5: one launch for all num_spk aligned speakers, on the same views
 * and into the same beamformer planes; with refine set it reads the refined images, so that V = Y - sum_s gamma_s Y is the noise
 * class's image.  opts == NULL: back to the per-speaker step that is set (misonet_bf_opts or WPD).  Legal between runs; the
 * workspace size depends on it (ask misonet_pipeline_workspace_bytes again).  MISONET_EINVAL for bad fields (as
 * misonet_beamform_joint, M = num_mic, S = num_spk).  With it not set every bit of every path, every workspace offset and the
 * workspace size are unchanged. */
int misonet_pipeline_set_joint(misonet_pipeline* p, const misonet_jbf_opts* opts);
long long misonet_pipeline_workspace_bytes(const misonet_pipeline* p, int B, int T);
/* mix_dev complex64 [B,M,T,F]; clean_dev complex64 [B,S,T,F] or NULL; out_dev complex64 [B,S,T,F] (MISO3);
 * optional outputs (may be NULL): bf_dev complex64 [B,S,T,F] (MVDR), miso1_dev complex64 [B,S,M,T,F] (aligned).
 * out_dev == NULL with miso1_dev != NULL runs the separation stage only (MISO1_Inference + alignments): the input of
 * the utterance-wise beamformer of Tester_Beamforming (tester.py:340-449). */
int misonet_pipeline_run(misonet_pipeline* p, const void* mix_dev, const void* clean_dev, int B, int T,
                         void* out_dev, void* bf_dev, void* miso1_dev, void* ws_dev, long long ws_bytes,
                         misonet_stream stream);
int misonet_pipeline_check(misonet_pipeline* p, const void* ws_dev, misonet_stream stream);
/* same pipeline fed with waveforms: wav_dev float32 [B, n_samples, M] (time-major, microphones interleaved: the
 * librosa.load(...).T array of dataloader/data.py:605-616), clean_wav_dev float32 [B, n_samples, S] (clean sources at
 * ref_ch) or NULL.  The STFT front-end (data.py:505-522,540-544) runs on the device straight into the kernels' layout;
 * T = n_samples/64 + 1 frames (misonet_pipeline_workspace_bytes takes that T). */
int misonet_pipeline_run_wav(misonet_pipeline* p, const float* wav_dev, const float* clean_wav_dev, int B,
                             int n_samples, void* out_dev, void* bf_dev, void* miso1_dev, void* ws_dev,
                             long long ws_bytes, misonet_stream stream);

/* ---- STFT front-end alone: AudioDataset_Test.STFT + "/scale" + permute (dataloader/data.py:505-522, 540-544) ------ */
/* wav_dev float32 [B, n_samples, M] -> out_dev complex64 [B, M, T, 129], T = n_samples/64 + 1: hann-256, hop 64,
 * zero boundary padding, un-normalised.  The twiddle tables (0.3 MB per device) are built by misonet_net_commit,
 * misonet_pipeline_create or misonet_frontend_init (ABI 430; see misonet_istft below for a process that calls none of them). */
int misonet_stft_frames(int n_samples);
long long misonet_stft_workspace_bytes(int B, int M, int n_samples);
/* STFT + iSTFT tables (0.3 MB) and kernel attributes of the CURRENT device; idempotent (ABI 430) */
int misonet_frontend_init(void);
int misonet_stft(const float* wav_dev, int B, int n_samples, int M, void* out_dev, void* ws_dev, long long ws_bytes,
                 misonet_stream stream);

/* ---- iSTFT + int16: Tester_Enhance.ISTFT and the post-processing of tester.py:949-952, 979-990 ("x scale" ->
 * scipy.signal.istft(hann, 256, 192) -> "x 32767" -> astype(int16)) (ABI 420) ---------------------------------------- */
/* spec_dev complex64 [N, T, 129] (the boundary layout of every output above, T >= 2) -> 64 (T - 1) samples per row:
 * out_i16_dev int16 [N, 64 (T - 1)] (truncating cast of y * 32767) and / or out_f32_dev float32 of the same shape (either
 * may be NULL).  The windowed inverse DFT runs on the fp32 matrix cores, overlap-add and the division by the window
 * envelope follow on chip.  Like every other call it is asynchronous and allocation-free -- PROVIDED the front-end tables of
 * the current device exist: misonet_net_commit, misonet_pipeline_create and misonet_frontend_init build them (hipMalloc +
 * synchronous copy, once per device, thread-safe).  A process that calls misonet_stft / misonet_istft without any of
 * these builds them inside its first call, which therefore synchronises and must not sit inside a stream capture. */
int misonet_istft(const void* spec_dev, int N, int T, void* out_i16_dev, float* out_f32_dev, misonet_stream stream);

/* ---- streaming STFT and iSTFT: waveform blocks in, frames out; frames in, waveform blocks out (ABI 650) ------------------
 * The two transforms above fed piece by piece, with their state on the device.  Window, hop, twiddles and
 * scaling are those above: periodic hann-256, hop 64, un-normalised, F = 129.  The bits do not depend on how a stream is cut
 * into calls, and a stream that ends with `flush` has emitted, concatenated, the result of misonet_stft / misonet_istft of
 * the whole signal BIT FOR BIT.
 *
 * Analysis.  A stream has seen N = n_seen samples per channel; X_t[f] = sum_{j<256} x[64 t - 128 + j] hann[j] e^{-2 pi i f j/256}
 * with x = 0 outside the samples that exist.  Frame t is complete once sample 64 t + 127 has arrived: after N samples the stream
 * has emitted e(N) = max(0, N / 64 - 1) frames.  A call with n_new samples emits the frames [e(N), E): E = e(N + n_new) without
 * flush, E = (N + n_new) / 64 + 1 with it (everything beyond sample N + n_new counts as zero, as misonet_stft treats
 * l >= n_samples).  misonet_stft_stream_frames returns E - e(N); it may be 0, and the call still advances the state.
 *   wav_dev    float32 [B, n_new, M], the layout of misonet_stft (may be NULL when n_new == 0)
 *   out_c64_dev complex64 [B, M, Tn, 129], Tn = misonet_stft_stream_frames(...), every element written (may be NULL when Tn == 0)
 *   state_dev  misonet_stft_stream_state_bytes(B, M) bytes: per (b, m) the last 255 samples of the stream, aligned to its end,
 *              zero where the stream has not begun (enough: 64 e(N) - 128 >= N - 255).  misonet_stft_stream_reset writes every
 *              byte with zeros.  After a flushing call the state is spent until the next reset.
 * Synthesis.  A stream of R rows has seen Tc = t_seen frames.  Output hop h covers the samples 64 h .. 64 h + 63 and needs the
 * frames h - 1 .. h + 2: after Tc frames the stream has emitted g(Tc) = max(0, Tc - 2) hops.  A call with t_new frames emits the
 * hops [g(Tc), G): G = g(Tc + t_new) without flush, G = max(0, Tc + t_new - 1) with it.  Per sample
 * y = sum w[k] z_t[k] / sum w[k]^2 over the frames t in {h - 1, h, h + 1, h + 2} that exist -- 0 <= t, and at a flush also
 * t < Tc + t_new -- t ascending, the quotient in float32, as misonet_istft.  A frame that does not exist is skipped, not added
 * as zero: only hop 0 and the flush hop have partial envelopes.  misonet_istft_stream_hops returns G - g(Tc).  A stream flushed
 * with fewer than 2 frames emits nothing.
 *   spec_dev   complex64 [R, t_new, 129] (may be NULL when t_new == 0)
 *   out_i16_dev / out_f32_dev  int16 / float32 [R, 64 H], H = misonet_istft_stream_hops(...): (short)(int)(y * 32767.0f) and / or
 *              y; either may be NULL, both when H == 0
 *   state_dev  misonet_istft_stream_state_bytes(R) bytes: per row the last 3 frames, complex64 [3][129]; reset writes zeros
 * The host passes n_seen (t_seen): the kernels keep no counter on the device.  A launch depends on them only through the ranges
 * above and through n_seen mod 64; for n_seen >= 128 (t_seen >= 3) on nothing else, so a steady-state call (say, blocks of 256
 * samples) can be captured into a HIP graph and replayed.  A call is one launch for the output (none when it emits nothing) and
 * one small launch behind it that moves the state on (none at a flush); no host synchronisation, no allocation, no atomics.
 * Limits: 1 <= B <= 65535, 1 <= M <= 64, 1 <= R <= 65535, 0 <= n_new <= 2^28, 0 <= t_new <= 2^22 (>= 1 unless flush), n_seen,
 * t_seen >= 0; anything else is MISONET_EINVAL (-1 from the count functions) before any launch and before any pointer is looked
 * at; a short state is MISONET_ENOMEM.  The tables are those of misonet_frontend_init: the first use on a device builds them
 * and must not sit inside a stream capture.
 * Latency: output sample 64 h needs input sample 64 h + 255 -- 255 samples for the pair, plus the block. */
long long misonet_stft_stream_state_bytes(int B, int M);
int misonet_stft_stream_reset(void* state_dev, int B, int M, misonet_stream stream);
long long misonet_stft_stream_frames(long long n_seen, long long n_new, int flush);      /* -1 on bad arguments */
int misonet_stft_stream(const float* wav_dev, int B, long long n_new, int M, long long n_seen, int flush, void* out_c64_dev,
                        void* state_dev, long long state_bytes, misonet_stream stream);
long long misonet_istft_stream_state_bytes(int R);
int misonet_istft_stream_reset(void* state_dev, int R, misonet_stream stream);
long long misonet_istft_stream_hops(long long t_seen, long long t_new, int flush);       /* -1 on bad arguments */
int misonet_istft_stream(const void* spec_dev, int R, long long t_new, long long t_seen, int flush, void* out_i16_dev,
                         float* out_f32_dev, void* state_dev, long long state_bytes, misonet_stream stream);

/* ---- per-launch timing (bench.py roofline leg): while enabled, the library brackets every conv launch, the TCN
 * section and the beamforming section of each forward with HIP events on the caller's stream.  kinds: 0 = 3x3 conv kernel
 * launches, 1 = TCN sections, 2 = beamforming sections (whichever beamformer is set), 3 = other (conv_wprep_k, the per-sample weight preparation of the
 * DMA dataflow).  State is per device (the current device at the call); misonet_profile_end synchronises and sums. */
int misonet_profile_begin(int max_launches);
int misonet_profile_end(double* ms_by_kind /*[4]*/, long long* launches_by_kind /*[4]*/);

/* ---- timing helper: HIP events on the caller's stream (bench.py roofline leg) ------------------------------- */
int misonet_event_create(void** ev);
int misonet_event_record(void* ev, misonet_stream stream);
int misonet_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on stop */
int misonet_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* MISONET_H_ */
