// C ABI of the array processing (include/misonet.h): the drop-in beamformers misonet_mvdr* / misonet_bf_* / misonet_beamform*
// (mvdr.hip), WPE dereverberation misonet_wpe* (wpe.hip) and its online form misonet_owpe* (owpe.hip), the WPD beamformer
// misonet_wpd* (wpd.hip), guided spatial clustering
// misonet_cacgmm* / misonet_masks_from_estimates (cacgmm.hip), the joint beamformers misonet_beamform_joint* (jbf.hip), blind
// separation misonet_auxiva* (iva.hip) and its online form misonet_oiva* (oiva.hip), the online beamformer misonet_obf* (obf.hip), PIT alignment misonet_pit_* (mvdr.hip) and continuous separation
// misonet_css_* (css.hip).  Host code only.
#include "api_common.hpp"

using namespace mn;

// host-side check of every field; M = the number of microphones ref_ch is counted in
int mn::bf_opts_check(const misonet_bf_opts* o, int M) {
  if (!o) return fail(MISONET_EINVAL, "null beamformer options");
  if (o->kind != BF_MVDR && o->kind != BF_SOUDEN && o->kind != BF_GEV)
    return fail(MISONET_EINVAL, "beamformer kind %d: 0 mvdr, 1 souden, 2 gev", o->kind);
  if (o->noise != 0 && o->noise != 1) return fail(MISONET_EINVAL, "beamformer noise %d: 0 residual, 1 mix", o->noise);
  if (!(o->condition >= 0.0) || !std::isfinite(o->condition))
    return fail(MISONET_EINVAL, "beamformer condition (gamma) must be finite and >= 0 (got %g)", o->condition);
  if (!(o->epsi >= 0.f) || !std::isfinite(o->epsi))
    return fail(MISONET_EINVAL, "beamformer epsi must be finite and >= 0 (got %g)", (double)o->epsi);
  if (o->ref_ch < 0 || o->ref_ch >= M)
    return fail(MISONET_EINVAL, "beamformer ref_ch %d outside [0, %d)", o->ref_ch, M);
  return MISONET_OK;
}

void mn::bf_opts_apply(const misonet_bf_opts& o, MvdrArgs& a) {
  a.epsi = o.epsi; a.kind = o.kind; a.noise_mix = o.noise; a.trace_norm = o.trace_normalize != 0; a.ban = o.ban != 0;
  a.bf_ref = o.ref_ch; a.condition = o.condition;
}

// WPD: every field, against M microphones and (T >= 0) against T frames.  The order K = M (taps + 1) is bounded by WPD_KMAX, the
// order the Gram scheme of wpd.hip reaches; the LDS of every such K fits (wpd_lds_bytes is checked all the same).
int mn::wpd_opts_check(const misonet_wpd_opts* o, int M, int T) {
  if (!o) return fail(MISONET_EINVAL, "null WPD options");
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (o->taps < 1 || (long long)M * ((long long)o->taps + 1) > WPD_KMAX)
    return fail(MISONET_EINVAL, "taps must be >= 1 and M * (taps + 1) <= %d (got taps %d, M %d)", WPD_KMAX, o->taps, M);
  if (wpd_lds_bytes(M, o->taps) > 160 * 1024)
    return fail(MISONET_EINVAL, "taps %d with M %d does not fit the 160 KB of LDS", o->taps, M);
  if (o->delay < 1) return fail(MISONET_EINVAL, "delay must be >= 1 (got %d)", o->delay);
  if (!(o->diag_load >= 0.0) || !std::isfinite(o->diag_load))
    return fail(MISONET_EINVAL, "diag_load must be finite and >= 0 (got %g)", o->diag_load);
  if (!(o->power_floor >= 0.0) || !std::isfinite(o->power_floor))
    return fail(MISONET_EINVAL, "power_floor must be finite and >= 0 (got %g)", o->power_floor);
  if (o->ref_ch < 0 || o->ref_ch >= M) return fail(MISONET_EINVAL, "WPD ref_ch %d outside [0, %d)", o->ref_ch, M);
  if (T >= 0 && (long long)T <= (long long)o->delay + o->taps - 1)
    return fail(MISONET_EINVAL, "T must be > delay + taps - 1 = %lld (got %d)", (long long)o->delay + o->taps - 1, T);
  return MISONET_OK;
}

void mn::wpd_opts_apply(const misonet_wpd_opts& o, WpdArgs& a) {
  a.taps = o.taps; a.delay = o.delay; a.ref = o.ref_ch; a.diag_load = o.diag_load; a.power_floor = o.power_floor;
}

// the dynamic-LDS attribute of wpd_bin_k: once per device, never inside an asynchronous call after that
int mn::wpd_ready() {
  static DeviceOnce latch;
  return latch.once([] { HIPCHK(wpd_init()); return (int)MISONET_OK; });
}

// cACGMM: every field (the geometry is checked by the calls)
int mn::cacgmm_opts_check(const misonet_cacgmm_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null clustering options");
  if (o->iterations < 0 || o->iterations > 1000)
    return fail(MISONET_EINVAL, "iterations must be in [0, 1000] (got %d)", o->iterations);
  if (o->prior != 0 && o->prior != 1) return fail(MISONET_EINVAL, "prior %d: 0 bin, 1 guided", o->prior);
  if (!(o->diag_load >= 0.0) || !std::isfinite(o->diag_load))
    return fail(MISONET_EINVAL, "diag_load must be finite and >= 0 (got %g)", o->diag_load);
  if (!(o->prior_floor >= 0.0) || !std::isfinite(o->prior_floor) || (o->prior == 1 && !(o->prior_floor > 0.0)))
    return fail(MISONET_EINVAL, "prior_floor must be finite and >= 0, and > 0 for the guided prior (got %g)", o->prior_floor);
  return MISONET_OK;
}

static int cacgmm_geometry(int B, int K, int F, int M) {
  if (B <= 0 || B > 65535 || F <= 0) return fail(MISONET_EINVAL, "B must be in [1, 65535] and F positive (got %d, %d)", B, F);
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (K < 2 || K > 5) return fail(MISONET_EINVAL, "K = speakers + 1 must be in [2, 5] (got %d)", K);
  return MISONET_OK;
}

// joint beamformers: every field, against M microphones and S speakers
int mn::jbf_opts_check(const misonet_jbf_opts* o, int M, int S) {
  if (!o) return fail(MISONET_EINVAL, "null joint beamformer options");
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (S < 1 || S > 4 || S > M) return fail(MISONET_EINVAL, "S must be in [1, 4] and <= M (got S %d, M %d)", S, M);
  if (o->kind != JBF_LCMV && o->kind != JBF_MWF && o->kind != JBF_R1MWF)
    return fail(MISONET_EINVAL, "joint beamformer kind %d: 0 lcmv, 1 mwf, 2 r1mwf", o->kind);
  if (o->noise != 0 && o->noise != 1) return fail(MISONET_EINVAL, "joint beamformer noise %d: 0 residual, 1 mix", o->noise);
  if (o->rtf != 0 && o->rtf != 1) return fail(MISONET_EINVAL, "joint beamformer rtf %d: 0 cw, 1 eig", o->rtf);
  if (o->kind != JBF_LCMV && (o->noise != 0 || o->rtf != 0))
    return fail(MISONET_EINVAL, "noise \"mix\" and rtf belong to kind lcmv: they must keep their defaults for kind %d", o->kind);
  if (!(o->diag_load >= 0.0) || !std::isfinite(o->diag_load))
    return fail(MISONET_EINVAL, "diag_load must be finite and >= 0 (got %g)", o->diag_load);
  if (o->kind == JBF_MWF && (!(o->mu > 0.0) || !std::isfinite(o->mu)))
    return fail(MISONET_EINVAL, "mu must be finite and > 0 for kind mwf (got %g)", o->mu);
  if (o->kind == JBF_R1MWF && (!(o->mu >= 0.0) || !std::isfinite(o->mu)))
    return fail(MISONET_EINVAL, "mu must be finite and >= 0 for kind r1mwf (got %g)", o->mu);
  if (o->ref_ch < 0 || o->ref_ch >= M) return fail(MISONET_EINVAL, "joint beamformer ref_ch %d outside [0, %d)", o->ref_ch, M);
  return MISONET_OK;
}

void mn::jbf_opts_apply(const misonet_jbf_opts& o, JbfArgs& a) {
  a.kind = o.kind; a.noise_mix = o.noise; a.rtf_eig = o.rtf; a.ref = o.ref_ch; a.mu = o.mu; a.diag_load = o.diag_load;
}

static int jbf_geometry(int B, int F) {
  if (B <= 0 || B > 65535 || F <= 0) return fail(MISONET_EINVAL, "B must be in [1, 65535] and F positive (got %d, %d)", B, F);
  return MISONET_OK;
}

// The drop-in beamformer call: src / mix complex64 [B,F,M,T], one source per item.  misonet_beamform passes the caller's options
// (checked here, the workspace sized by their kind); misonet_mvdr passes the defaults with its epsi as trusted: that entry point
// has never validated epsi, and its workspace is misonet_mvdr_workspace_bytes.
static int beamform_dropin(const void* src, const void* mix, int B, int F, int M, int T, const misonet_bf_opts* opts,
                           bool trusted, void* out, void* ws, long long ws_bytes, misonet_stream stream) {
  if (!src || !mix || !out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (B <= 0 || F <= 0 || T <= 0) return fail(MISONET_EINVAL, "B, F, T must be positive");
  if (!trusted) { int r = bf_opts_check(opts, M); if (r) return r; }
  if (ws_bytes < (trusted ? mvdr_ws_bytes(B, 1, F, M) : bf_ws_bytes(B, 1, F, M, opts->kind)))
    return fail(MISONET_ENOMEM, "workspace too small");
  MvdrArgs a;
  const float* y = reinterpret_cast<const float*>(mix);
  const float* x = reinterpret_cast<const float*>(src);
  a.mix = {y, y + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.src = {x, x + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.est = nullptr; a.est_bstride = 0; a.sel = nullptr;
  a.S = 1; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = T;
  bf_opts_apply(*opts, a);
  float* o = reinterpret_cast<float*>(out);
  COut co = {o, o + 1, 2LL * T * F, 0, 2LL * F, 2};      // [B,T,F] complex64 (tester.py:1134)
  HIPCHK(launch_mvdr(a, co, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

extern "C" {

// ---- MVDR / PIT drop-in entry points ---------------------------------------------------------------------------
long long misonet_mvdr_workspace_bytes(int B, int F, int M) { return mvdr_ws_bytes(B, 1, F, M); }

int misonet_mvdr(const void* src, const void* mix, int B, int F, int M, int T, float epsi, void* out, void* ws,
                 long long ws_bytes, misonet_stream stream) {
  misonet_bf_opts o;
  misonet_bf_opts_default(&o);
  o.epsi = epsi;
  return beamform_dropin(src, mix, B, F, M, T, &o, true, out, ws, ws_bytes, stream);
}

int misonet_mvdr_debug(const void* ws, int B, int F, int M, void* steer, void* w, misonet_stream stream) {
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_mvdr_debug(ws, B, 1, F, M, reinterpret_cast<double*>(steer), reinterpret_cast<double*>(w),
                           reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- selectable beamformers (ABI 510) ------------------------------------------------------------------------------
int misonet_bf_opts_default(misonet_bf_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->kind = BF_MVDR; o->noise = 0; o->condition = 0.0; o->trace_normalize = 0; o->epsi = 1e-6f; o->ban = 0; o->ref_ch = 0;
  return MISONET_OK;
}

long long misonet_beamform_workspace_bytes(int B, int F, int M, const misonet_bf_opts* opts) {
  if (B <= 0 || F <= 0 || M < 2 || M > 8 || bf_opts_check(opts, M)) return -1;
  return bf_ws_bytes(B, 1, F, M, opts->kind);
}

int misonet_beamform(const void* src, const void* mix, int B, int F, int M, int T, const misonet_bf_opts* opts, void* out,
                     void* ws, long long ws_bytes, misonet_stream stream) {
  return beamform_dropin(src, mix, B, F, M, T, opts, false, out, ws, ws_bytes, stream);
}

int misonet_beamform_debug(const void* ws, int B, int F, int M, const misonet_bf_opts* opts, void* w, double* lam,
                           misonet_stream stream) {
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  if (B <= 0 || F <= 0 || M < 2 || M > 8) return fail(MISONET_EINVAL, "B, F must be positive and M in [2, 8]");
  { int r = bf_opts_check(opts, M); if (r) return r; }
  if (lam && opts->kind != BF_GEV) return fail(MISONET_EINVAL, "lambda_max exists for kind gev only");
  HIPCHK(launch_bf_debug(ws, B, 1, F, M, reinterpret_cast<double*>(w), lam, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- WPE dereverberation (ABI 520) ---------------------------------------------------------------------------------
int misonet_wpe_opts_default(misonet_wpe_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->taps = 10; o->delay = 3; o->iterations = 3; o->diag_load = 0.0; o->power_floor = 1e-10;
  return MISONET_OK;
}

// host-side check of every field and of the geometry they are used with
static int wpe_check(int B, int M, int T, int F, const misonet_wpe_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null dereverberation options");
  if (B < 1 || F < 1) return fail(MISONET_EINVAL, "B and F must be positive (got %d, %d)", B, F);
  if (T < 2) return fail(MISONET_EINVAL, "T must be >= 2 (got %d)", T);
  if (M < 1 || M > 8) return fail(MISONET_EINVAL, "M must be in [1, 8] (got %d)", M);
  if (o->taps < 1 || (long long)M * o->taps > 80)
    return fail(MISONET_EINVAL, "taps must be >= 1 and M * taps <= 80 (got taps %d, M %d)", o->taps, M);
  if (o->delay < 1) return fail(MISONET_EINVAL, "delay must be >= 1 (got %d)", o->delay);
  if (o->iterations < 1 || o->iterations > 10) return fail(MISONET_EINVAL, "iterations must be in [1, 10] (got %d)", o->iterations);
  if (!(o->diag_load >= 0.0) || !std::isfinite(o->diag_load))
    return fail(MISONET_EINVAL, "diag_load must be finite and >= 0 (got %g)", o->diag_load);
  if (!(o->power_floor >= 0.0) || !std::isfinite(o->power_floor))
    return fail(MISONET_EINVAL, "power_floor must be finite and >= 0 (got %g)", o->power_floor);
  return MISONET_OK;
}

long long misonet_wpe_workspace_bytes(int B, int M, int T, int F, const misonet_wpe_opts* opts) {
  if (wpe_check(B, M, T, F, opts)) return -1;
  return wpe_ws_bytes(B, M, T, F, opts->taps);
}

int misonet_wpe(const void* mix, const float* power, int B, int M, int T, int F, const misonet_wpe_opts* opts, void* out,
                void* ws, long long ws_bytes, misonet_stream stream) {
  if (!mix || !out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (out == mix) return fail(MISONET_EINVAL, "out_dev must not be mix_dev");
  { int r = wpe_check(B, M, T, F, opts); if (r) return r; }
  if (ws_bytes < wpe_ws_bytes(B, M, T, F, opts->taps)) return fail(MISONET_ENOMEM, "workspace too small");
  HIPCHK(launch_wpe(mix, power, B, M, T, F, opts->taps, opts->delay, opts->iterations, opts->diag_load, opts->power_floor, out,
                    ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_wpe_debug(const void* ws, int B, int M, int F, const misonet_wpe_opts* opts, void* g, int* fail_dev,
                      misonet_stream stream) {
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  { int r = wpe_check(B, M, 2, F, opts); if (r) return r; }
  HIPCHK(launch_wpe_debug(ws, B, M, F, opts->taps, g, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- online WPE: frame-recursive, state carried (ABI 620) ------------------------------------------------------------
int misonet_owpe_opts_default(misonet_owpe_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->taps = 10; o->delay = 3; o->context = 0; o->alpha = 0.999; o->power_floor = 1e-10; o->init = 1.0;
  return MISONET_OK;
}

// host-side check of every field and of the geometry they are used with
static int owpe_check(int B, int M, int F, const misonet_owpe_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null online dereverberation options");
  if (B < 1 || F < 1 || (long long)B * F > 0x7fffffffLL)
    return fail(MISONET_EINVAL, "B and F must be positive with B * F < 2^31 (got %d, %d)", B, F);
  if (M < 1 || M > 8) return fail(MISONET_EINVAL, "M must be in [1, 8] (got %d)", M);
  if (o->taps < 1 || (long long)M * o->taps > 80)
    return fail(MISONET_EINVAL, "taps must be >= 1 and M * taps <= 80 (got taps %d, M %d)", o->taps, M);
  if (o->delay < 1) return fail(MISONET_EINVAL, "delay must be >= 1 (got %d)", o->delay);
  if (owpe_lds_bytes(M, o->taps, o->delay) > OWPE_LDS_LIMIT)
    return fail(MISONET_EINVAL, "delay %d with taps %d and M %d: the frame ring does not fit the 160 KB of LDS", o->delay, o->taps, M);
  if (o->context < 0 || o->context > OWPE_CTX)
    return fail(MISONET_EINVAL, "context must be in [0, %d] (got %d)", OWPE_CTX, o->context);
  if (!(o->alpha > 0.0 && o->alpha <= 1.0)) return fail(MISONET_EINVAL, "alpha must be in (0, 1] (got %g)", o->alpha);
  if (!pos_finite(o->power_floor)) return fail(MISONET_EINVAL, "power_floor must be finite and > 0 (got %g)", o->power_floor);
  if (!pos_finite(o->init)) return fail(MISONET_EINVAL, "init must be finite and > 0 (got %g)", o->init);
  return MISONET_OK;
}

// the dynamic-LDS attribute of owpe_k: once per device, never inside an asynchronous call after that
static int owpe_ready() {
  static DeviceOnce latch;
  return latch.once([] { HIPCHK(owpe_init()); return (int)MISONET_OK; });
}

long long misonet_owpe_state_bytes(int B, int M, int F, const misonet_owpe_opts* opts) {
  if (owpe_check(B, M, F, opts)) return -1;
  return owpe_state_bytes((long long)B * F, M, opts->taps, opts->delay);
}

int misonet_owpe_lds_bytes(int M, const misonet_owpe_opts* opts) {
  if (owpe_check(1, M, 1, opts)) return -1;
  return (int)owpe_lds_bytes(M, opts->taps, opts->delay);
}

int misonet_owpe_reset(void* state, int B, int M, int F, const misonet_owpe_opts* opts, misonet_stream stream) {
  if (!state) return fail(MISONET_EINVAL, "null argument");
  { int r = owpe_check(B, M, F, opts); if (r) return r; }
  { int r = owpe_ready(); if (r) return r; }
  HIPCHK(launch_owpe_reset(state, B, M, F, opts->taps, opts->delay, opts->init, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_owpe(const void* mix, int B, int M, int T, int F, const misonet_owpe_opts* opts, void* out, void* state,
                 long long state_bytes, misonet_stream stream) {
  if (!mix || !out || !state) return fail(MISONET_EINVAL, "null argument");
  if (out == mix) return fail(MISONET_EINVAL, "out_dev must not be mix_dev");
  { int r = owpe_check(B, M, F, opts); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be >= 1 (got %d)", T);
  if (state_bytes < owpe_state_bytes((long long)B * F, M, opts->taps, opts->delay))
    return fail(MISONET_ENOMEM, "state too small");
  { int r = owpe_ready(); if (r) return r; }
  HIPCHK(launch_owpe(mix, B, M, T, F, opts->taps, opts->delay, opts->context, opts->alpha, opts->power_floor, out, state,
                     reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_owpe_debug(const void* state, int B, int M, int F, const misonet_owpe_opts* opts, void* g, void* p, int* fail_dev,
                       int* n_dev, misonet_stream stream) {
  if (!state) return fail(MISONET_EINVAL, "null argument");
  { int r = owpe_check(B, M, F, opts); if (r) return r; }
  HIPCHK(launch_owpe_debug(state, B, M, F, opts->taps, opts->delay, g, p, fail_dev, n_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- online AuxIVA: frame-recursive separation, state carried (ABI 630) ----------------------------------------------
int misonet_oiva_opts_default(misonet_oiva_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->model = 0; o->ref_ch = 0; o->alpha = 0.98; o->floor = 1e-10; o->init = 1.0;
  return MISONET_OK;
}

static int oiva_geom_check(int B, int M, int F) {
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (B < 1) return fail(MISONET_EINVAL, "B must be positive (got %d)", B);
  if (F < 1 || F > 1025) return fail(MISONET_EINVAL, "F must be in [1, 1025] (got %d)", F);
  if ((long long)B * F > 0x7fffffffLL) return fail(MISONET_EINVAL, "B * F must be < 2^31 (got %d, %d)", B, F);
  return MISONET_OK;
}

// host-side check of every field and of the geometry they are used with
static int oiva_check(int B, int M, int F, const misonet_oiva_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null online separation options");
  { int r = oiva_geom_check(B, M, F); if (r) return r; }
  if (o->model != 0 && o->model != 1) return fail(MISONET_EINVAL, "model %d: 0 gauss, 1 laplace", o->model);
  if (o->ref_ch < 0 || o->ref_ch >= M) return fail(MISONET_EINVAL, "ref_ch %d outside [0, %d)", o->ref_ch, M);
  if (!in_open_unit(o->alpha))
    return fail(MISONET_EINVAL, "alpha must be in (0, 1): 1 would freeze the covariances (got %g)", o->alpha);
  if (!pos_finite(o->floor)) return fail(MISONET_EINVAL, "floor must be finite and > 0 (got %g)", o->floor);
  if (!pos_finite(o->init)) return fail(MISONET_EINVAL, "init must be finite and > 0 (got %g)", o->init);
  return MISONET_OK;
}

long long misonet_oiva_state_bytes(int B, int M, int F) {
  if (oiva_geom_check(B, M, F)) return -1;
  return oiva_state_bytes((long long)B * F, M);
}

int misonet_oiva_bins_per_pass(int M) {
  if (M < 2 || M > 8) { fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M); return -1; }
  return oiva_bins_per_pass(M);
}

int misonet_oiva_reset(void* state, int B, int M, int F, const misonet_oiva_opts* opts, misonet_stream stream) {
  { int r = oiva_check(B, M, F, opts); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_oiva_reset(state, B, M, F, opts->init, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_oiva(const void* mix, int B, int M, int T, int F, const misonet_oiva_opts* opts, void* est, void* images, void* state,
                 long long state_bytes, misonet_stream stream) {
  { int r = oiva_check(B, M, F, opts); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be >= 1 (got %d)", T);
  if (!mix || !est || !state) return fail(MISONET_EINVAL, "null argument");
  // the 128-bit predicate of misonet_obf.  For every block that fits the address space (n M < 2^63) the 64-bit comparison this
  // call used before never wrapped, and the two agree
  const unsigned __int128 n = (unsigned __int128)B * M * T * F * 8;
  if (ranges_overlap(mix, n, est, n) || (images && (ranges_overlap(mix, n, images, n * M) || ranges_overlap(est, n, images, n * M))))
    return fail(MISONET_EINVAL, "mix_dev, est_out_dev and images_out_dev must not overlap");
  if (state_bytes < oiva_state_bytes((long long)B * F, M)) return fail(MISONET_ENOMEM, "state too small");
  HIPCHK(launch_oiva(mix, B, M, T, F, opts->model, opts->ref_ch, opts->alpha, opts->floor, est, images, state,
                     reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_oiva_debug(const void* state, int B, int M, int F, void* w, void* v, int* fail_dev, int* n_dev, misonet_stream stream) {
  { int r = oiva_geom_check(B, M, F); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_oiva_debug(state, B, M, F, w, v, fail_dev, n_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- online AuxIVA for fewer sources than microphones: K rows, state carried (ABI 670) ------------------------------------
static int overiva_geom_check(int B, int M, int K, int F) {
  { int r = oiva_geom_check(B, M, F); if (r) return r; }
  if (K == M) return fail(MISONET_EINVAL, "K = M = %d is the determined case: that is misonet_oiva", M);
  if (K < 1 || K > M) return fail(MISONET_EINVAL, "K must be in [1, M - 1] = [1, %d] (got %d)", M - 1, K);
  return MISONET_OK;
}

static int overiva_check(int B, int M, int K, int F, const misonet_oiva_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null online separation options");
  { int r = overiva_geom_check(B, M, K, F); if (r) return r; }
  return oiva_check(B, M, F, o);
}

long long misonet_overiva_state_bytes(int B, int M, int K, int F) {
  if (overiva_geom_check(B, M, K, F)) return -1;
  return overiva_state_bytes((long long)B * F, M, K);
}

int misonet_overiva_bins_per_pass(int M, int K) {
  if (M < 2 || M > 8) { fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M); return -1; }
  if (K == M) { fail(MISONET_EINVAL, "K = M = %d is the determined case: that is misonet_oiva_bins_per_pass", M); return -1; }
  if (K < 1 || K > M) { fail(MISONET_EINVAL, "K must be in [1, M - 1] = [1, %d] (got %d)", M - 1, K); return -1; }
  return overiva_bins_per_pass(M, K);
}

int misonet_overiva_reset(void* state, int B, int M, int K, int F, const misonet_oiva_opts* opts, misonet_stream stream) {
  { int r = overiva_check(B, M, K, F, opts); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_overiva_reset(state, B, M, K, F, opts->init, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_overiva(const void* mix, int B, int M, int K, int T, int F, const misonet_oiva_opts* opts, void* est, void* images,
                    void* state, long long state_bytes, misonet_stream stream) {
  { int r = overiva_check(B, M, K, F, opts); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be >= 1 (got %d)", T);
  if (!mix || !est || !state) return fail(MISONET_EINVAL, "null argument");
  const unsigned __int128 n = (unsigned __int128)B * T * F * 8;             // one microphone or one source of the block
  if (ranges_overlap(mix, n * M, est, n * K) ||
      (images && (ranges_overlap(mix, n * M, images, n * K * M) || ranges_overlap(est, n * K, images, n * K * M))))
    return fail(MISONET_EINVAL, "mix_dev, est_out_dev and images_out_dev must not overlap");
  if (state_bytes < overiva_state_bytes((long long)B * F, M, K)) return fail(MISONET_ENOMEM, "state too small");
  HIPCHK(launch_overiva(mix, B, M, K, T, F, opts->model, opts->ref_ch, opts->alpha, opts->floor, est, images, state,
                        reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_overiva_debug(const void* state, int B, int M, int K, int F, void* ws, void* j, void* v, void* c, int* fail_dev,
                          int* n_dev, misonet_stream stream) {
  { int r = overiva_geom_check(B, M, K, F); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_overiva_debug(state, B, M, K, F, ws, j, v, c, fail_dev, n_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- online beamformer: frame-recursive MVDR / MWF, state carried (ABI 640) ---------------------------------------------
int misonet_obf_opts_default(misonet_obf_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->noise = 0; o->ref_ch = 0; o->alpha = 0.98; o->mu = 0.0; o->diag_load = 1e-3; o->epsi = 1e-10; o->init = 1.0;
  return MISONET_OK;
}

static int obf_geom_check(int B, int S, int M, int F) {
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (S < 1 || S > 8) return fail(MISONET_EINVAL, "S must be in [1, 8] (got %d)", S);
  if (B < 1) return fail(MISONET_EINVAL, "B must be positive (got %d)", B);
  if (F < 1 || F > 1025) return fail(MISONET_EINVAL, "F must be in [1, 1025] (got %d)", F);
  if ((long long)B * S * F > 0x7fffffffLL) return fail(MISONET_EINVAL, "B * S * F must be < 2^31 (got %d, %d, %d)", B, S, F);
  return MISONET_OK;
}

// host-side check of every field and of the geometry they are used with
static int obf_check(int B, int S, int M, int F, const misonet_obf_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null online beamformer options");
  { int r = obf_geom_check(B, S, M, F); if (r) return r; }
  if (o->noise != 0 && o->noise != 1) return fail(MISONET_EINVAL, "noise %d: 0 residual, 1 mix", o->noise);
  if (o->ref_ch < 0 || o->ref_ch >= M) return fail(MISONET_EINVAL, "ref_ch %d outside [0, %d)", o->ref_ch, M);
  if (!in_open_unit(o->alpha))
    return fail(MISONET_EINVAL, "alpha must be in (0, 1): 1 would freeze the covariances (got %g)", o->alpha);
  if (!nonneg_finite(o->mu)) return fail(MISONET_EINVAL, "mu must be finite and >= 0 (got %g)", o->mu);
  if (!nonneg_finite(o->diag_load)) return fail(MISONET_EINVAL, "diag_load must be finite and >= 0 (got %g)", o->diag_load);
  if (!nonneg_finite(o->epsi)) return fail(MISONET_EINVAL, "epsi must be finite and >= 0 (got %g)", o->epsi);
  if (!nonneg_finite(o->init)) return fail(MISONET_EINVAL, "init must be finite and >= 0 (got %g)", o->init);
  return MISONET_OK;
}

long long misonet_obf_state_bytes(int B, int S, int M, int F) {
  if (obf_geom_check(B, S, M, F)) return -1;
  return obf_state_bytes((long long)B * S * F, M);
}

int misonet_obf_cells_per_block(int M) {
  if (M < 2 || M > 8) { fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M); return -1; }
  return obf_cells_per_block(M);
}

int misonet_obf_reset(void* state, int B, int S, int M, int F, const misonet_obf_opts* opts, misonet_stream stream) {
  { int r = obf_check(B, S, M, F, opts); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_obf_reset(state, B, S, M, F, opts->init, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_obf(const void* mix, const void* images, int B, int S, int M, int T, int F, const misonet_obf_opts* opts, void* out,
                void* state, long long state_bytes, misonet_stream stream) {
  { int r = obf_check(B, S, M, F, opts); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be >= 1 (got %d)", T);
  if (!mix || !images || !out || !state) return fail(MISONET_EINVAL, "null argument");
  const long long need = obf_state_bytes((long long)B * S * F, M);
  const unsigned __int128 plane = (unsigned __int128)B * T * F * 8, nm = plane * M, no = plane * S, ni = no * M;
  const unsigned __int128 ns = (unsigned __int128)(state_bytes < need ? (state_bytes > 0 ? state_bytes : 0) : need);
  if (ranges_overlap(mix, nm, images, ni) || ranges_overlap(mix, nm, out, no) || ranges_overlap(images, ni, out, no) ||
      ranges_overlap(state, ns, mix, nm) || ranges_overlap(state, ns, images, ni) || ranges_overlap(state, ns, out, no))
    return fail(MISONET_EINVAL, "mix_dev, images_dev, out_dev and state_dev must not overlap");
  if (state_bytes < need) return fail(MISONET_ENOMEM, "state too small");
  HIPCHK(launch_obf(mix, images, B, S, M, T, F, opts->noise, opts->ref_ch, opts->alpha, opts->mu, opts->diag_load, opts->epsi, out,
                    state, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_obf_debug(const void* state, int B, int S, int M, int F, void* phi_s, void* phi_n, void* w, int* fail_dev, int* n_dev,
                      misonet_stream stream) {
  { int r = obf_geom_check(B, S, M, F); if (r) return r; }
  if (!state) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_obf_debug(state, B, S, M, F, phi_s, phi_n, w, fail_dev, n_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- WPD convolutional beamformer (ABI 530) --------------------------------------------------------------------------
int misonet_wpd_opts_default(misonet_wpd_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->taps = 5; o->delay = 3; o->diag_load = 0.0; o->power_floor = 1e-10; o->ref_ch = 0;
  return MISONET_OK;
}

long long misonet_wpd_workspace_bytes(int B, int F, int M, const misonet_wpd_opts* opts) {
  if (B <= 0 || F <= 0) { fail(MISONET_EINVAL, "B and F must be positive (got %d, %d)", B, F); return -1; }
  if (wpd_opts_check(opts, M, -1)) return -1;
  return wpd_ws_bytes(B, 1, F, M, opts->taps);
}

int misonet_wpd(const void* src, const void* mix, int B, int F, int M, int T, const misonet_wpd_opts* opts, void* out, void* ws,
                long long ws_bytes, misonet_stream stream) {
  if (B <= 0 || F <= 0 || T <= 0) return fail(MISONET_EINVAL, "B, F, T must be positive");
  { int r = wpd_opts_check(opts, M, T); if (r) return r; }
  if (!src || !mix || !out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (ws_bytes < wpd_ws_bytes(B, 1, F, M, opts->taps)) return fail(MISONET_ENOMEM, "workspace too small");
  { int r = wpd_ready(); if (r) return r; }
  WpdArgs a;
  const float* y = reinterpret_cast<const float*>(mix);
  const float* x = reinterpret_cast<const float*>(src);
  a.mix = {y, y + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.src = {x, x + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.est = nullptr; a.est_bstride = 0; a.sel = nullptr;
  a.S = 1; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = T;
  wpd_opts_apply(*opts, a);
  float* o = reinterpret_cast<float*>(out);
  COut co = {o, o + 1, 2LL * T * F, 0, 2LL * F, 2};      // [B,T,F] complex64, as misonet_beamform
  HIPCHK(launch_wpd(a, co, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_wpd_debug(const void* ws, int B, int F, int M, const misonet_wpd_opts* opts, void* wbar, int* fail_dev,
                      misonet_stream stream) {
  if (B <= 0 || F <= 0) return fail(MISONET_EINVAL, "B and F must be positive (got %d, %d)", B, F);
  { int r = wpd_opts_check(opts, M, -1); if (r) return r; }
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_wpd_debug(ws, B, 1, F, M, opts->taps, wbar, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- guided spatial clustering, cACGMM (ABI 560) -----------------------------------------------------------------------
int misonet_cacgmm_opts_default(misonet_cacgmm_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->iterations = 10; o->prior = 0; o->diag_load = 1e-8; o->prior_floor = 1e-6;
  return MISONET_OK;
}

long long misonet_cacgmm_workspace_bytes(int B, int K, int F, int M) {
  if (cacgmm_geometry(B, K, F, M)) return -1;
  return cacgmm_ws_bytes(B, K, F, M);
}

int misonet_cacgmm(const void* mix, const float* init_masks, int B, int K, int F, int M, int T, const misonet_cacgmm_opts* opts,
                   float* masks_out, void* images_out, void* ws, long long ws_bytes, misonet_stream stream) {
  { int r = cacgmm_geometry(B, K, F, M); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be positive (got %d)", T);
  { int r = cacgmm_opts_check(opts); if (r) return r; }
  if (!mix || !init_masks || !masks_out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (masks_out == init_masks) return fail(MISONET_EINVAL, "masks_out must not be init_masks (the initial masks are read in every sweep)");
  if (ws_bytes < cacgmm_ws_bytes(B, K, F, M)) return fail(MISONET_ENOMEM, "workspace too small");
  CacgmmArgs a;
  const float* y = reinterpret_cast<const float*>(mix);
  a.mix = {y, y + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.init = init_masks; a.masks = masks_out;
  float* o = reinterpret_cast<float*>(images_out);
  const int S = K - 1;
  a.img = {o, o ? o + 1 : nullptr, 2LL * S * F * M * T, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2, T};   // [B,S,F,M,T] complex64
  a.B = B; a.K = K; a.F = F; a.M = M; a.T = T;
  a.iters = opts->iterations; a.guided = opts->prior; a.diag_load = opts->diag_load; a.prior_floor = opts->prior_floor;
  HIPCHK(launch_cacgmm(a, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_cacgmm_debug(const void* ws, int B, int K, int F, int M, void* bk, double* pi, double* ll, int* fail_dev,
                         misonet_stream stream) {
  { int r = cacgmm_geometry(B, K, F, M); if (r) return r; }
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_cacgmm_debug(ws, B, K, F, M, bk, pi, ll, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_masks_from_estimates(const void* est, const void* mix, int B, int S, int F, int M, int T, float* masks_out,
                                 misonet_stream stream) {
  { int r = cacgmm_geometry(B, S + 1, F, M); if (r) return r; }
  if (F > 65535) return fail(MISONET_EINVAL, "F must be <= 65535 (got %d)", F);
  if (T < 1) return fail(MISONET_EINVAL, "T must be positive (got %d)", T);
  if (!est || !mix || !masks_out) return fail(MISONET_EINVAL, "null argument");
  MaskArgs a;
  const float* y = reinterpret_cast<const float*>(mix);
  const float* x = reinterpret_cast<const float*>(est);
  a.mix = {y, y + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.src = {x, x + 1, 2LL * S * F * M * T, 2LL * M * T, 2LL * T, 2};                  // [B,S,F,M,T] complex64
  a.src_ss = 2LL * F * M * T;
  a.est = nullptr; a.est_bstride = 0; a.sel = nullptr;
  a.S = S; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = T;
  a.masks = masks_out;
  HIPCHK(launch_masks_from_est(a, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- joint multi-speaker beamformers: LCMV, SDW-MWF, rank-1 MWF (ABI 570) ------------------------------------------------
int misonet_jbf_opts_default(misonet_jbf_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->kind = JBF_LCMV; o->noise = 0; o->rtf = 0; o->mu = 1.0; o->diag_load = 0.0; o->ref_ch = 0;
  return MISONET_OK;
}

long long misonet_beamform_joint_workspace_bytes(int B, int S, int F, int M, const misonet_jbf_opts* opts) {
  if (jbf_geometry(B, F) || jbf_opts_check(opts, M, S)) return -1;
  return jbf_ws_bytes(B, S, F, M, opts->kind);
}

int misonet_beamform_joint(const void* src, const void* mix, int B, int S, int F, int M, int T, const misonet_jbf_opts* opts,
                           void* out, void* ws, long long ws_bytes, misonet_stream stream) {
  { int r = jbf_geometry(B, F); if (r) return r; }
  if (T < 1) return fail(MISONET_EINVAL, "T must be positive (got %d)", T);
  { int r = jbf_opts_check(opts, M, S); if (r) return r; }
  if (!src || !mix || !out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (ws_bytes < jbf_ws_bytes(B, S, F, M, opts->kind)) return fail(MISONET_ENOMEM, "workspace too small");
  JbfArgs a;
  const float* y = reinterpret_cast<const float*>(mix);
  const float* x = reinterpret_cast<const float*>(src);
  a.mix = {y, y + 1, 2LL * F * M * T, 2LL * M * T, 2LL * T, 2};
  a.src = {x, x + 1, 2LL * S * F * M * T, 2LL * M * T, 2LL * T, 2};                  // [B,S,F,M,T] complex64
  a.src_ss = 2LL * F * M * T;
  a.est = nullptr; a.est_bstride = 0; a.sel = nullptr;
  a.S = S; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = T;
  jbf_opts_apply(*opts, a);
  float* o = reinterpret_cast<float*>(out);
  COut co = {o, o + 1, 2LL * S * T * F, 2LL * T * F, 2LL * F, 2};                    // [B,S,T,F] complex64
  HIPCHK(launch_jbf(a, co, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_beamform_joint_debug(const void* ws, int B, int S, int F, int M, const misonet_jbf_opts* opts, void* w, void* rtf,
                                 int* fail_dev, misonet_stream stream) {
  { int r = jbf_geometry(B, F); if (r) return r; }
  { int r = jbf_opts_check(opts, M, S); if (r) return r; }
  if (rtf && opts->kind != JBF_LCMV) return fail(MISONET_EINVAL, "the relative transfer functions exist for kind lcmv only");
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_jbf_debug(ws, B, S, F, M, opts->kind, w, rtf, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- blind separation, AuxIVA-ISS (ABI 580) ---------------------------------------------------------------------------
int misonet_iva_opts_default(misonet_iva_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->iterations = 20; o->model = 0; o->channels = 0; o->ref_ch = 0; o->floor = 1e-10;
  return MISONET_OK;
}

// the geometry; K = the channels after the PCA (already resolved: never 0 here)
static int iva_geometry(int B, int S, int K, int F, int M, int T) {
  if (B <= 0 || F <= 0 || T <= 0) return fail(MISONET_EINVAL, "B, F and T must be positive (got %d, %d, %d)", B, F, T);
  if (M < 2 || M > 8) return fail(MISONET_EINVAL, "M must be in [2, 8] (got %d)", M);
  if (S < 1 || S > 4 || S > M) return fail(MISONET_EINVAL, "S must be in [1, min(M, 4)] (got S %d, M %d)", S, M);
  if (K < S || K > M) return fail(MISONET_EINVAL, "channels must be in [S, M] = [%d, %d] (got %d)", S, M, K);
  if ((long long)B * F > 0x7fffffffLL || (long long)B * K > 0x7fffffffLL || T > 65535 * 256)
    return fail(MISONET_EINVAL, "B F, B channels and T / 256 must fit a launch grid (got B %d, F %d, T %d)", B, F, T);
  return MISONET_OK;
}

static int iva_opts_check(const misonet_iva_opts* o, int S, int M) {
  if (!o) return fail(MISONET_EINVAL, "null separation options");
  if (o->iterations < 0 || o->iterations > 1000)
    return fail(MISONET_EINVAL, "iterations must be in [0, 1000] (got %d)", o->iterations);
  if (o->model != 0 && o->model != 1) return fail(MISONET_EINVAL, "model %d: 0 gauss, 1 laplace", o->model);
  if (o->channels != 0 && (o->channels < S || o->channels > M))
    return fail(MISONET_EINVAL, "channels must be 0 (= S) or in [S, M] = [%d, %d] (got %d)", S, M, o->channels);
  if (o->ref_ch < 0 || o->ref_ch >= M) return fail(MISONET_EINVAL, "separation ref_ch %d outside [0, %d)", o->ref_ch, M);
  if (!(o->floor > 0.0) || !std::isfinite(o->floor)) return fail(MISONET_EINVAL, "floor must be finite and > 0 (got %g)", o->floor);
  return MISONET_OK;
}

long long misonet_auxiva_workspace_bytes(int B, int S, int K, int F, int M, int T) {
  if (iva_geometry(B, S, K, F, M, T)) return -1;
  return iva_ws_bytes(B, K, F, M, T);
}

int misonet_auxiva_resident_frames(int K) { return iva_resident_frames(K); }

int misonet_auxiva(const void* mix, int B, int S, int F, int M, int T, const misonet_iva_opts* opts, void* images_out,
                   int* order_out, void* ws, long long ws_bytes, misonet_stream stream) {
  { int r = iva_geometry(B, S, S, F, M, T); if (r) return r; }
  { int r = iva_opts_check(opts, S, M); if (r) return r; }
  const int K = opts->channels ? opts->channels : S;
  { int r = iva_geometry(B, S, K, F, M, T); if (r) return r; }
  if (!mix || !images_out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (ws_bytes < iva_ws_bytes(B, K, F, M, T)) return fail(MISONET_ENOMEM, "workspace too small");
  IvaArgs a;
  a.mix = mix; a.images = images_out; a.order_out = order_out;
  a.B = B; a.S = S; a.K = K; a.F = F; a.M = M; a.T = T;
  a.iters = opts->iterations; a.laplace = opts->model; a.ref = opts->ref_ch; a.floor = opts->floor;
  HIPCHK(launch_auxiva(a, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_auxiva_debug(const void* ws, int B, int K, int F, int M, int T, void* y, void* a, void* evec, double* power,
                         int* fail_dev, misonet_stream stream) {
  { int r = iva_geometry(B, 1, K, F, M, T); if (r) return r; }
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_auxiva_debug(ws, B, K, F, M, T, y, a, evec, power, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- room simulator (room.hip) ---------------------------------------------------------------------------------------------
static int room_geometry(int B, int S, int M, int Lh) {
  if (B < 1 || B > ROOM_MAX_B) return fail(MISONET_EINVAL, "B must be in [1, %d] (got %d)", ROOM_MAX_B, B);
  if (S < 1 || S > ROOM_MAX_S) return fail(MISONET_EINVAL, "S must be in [1, %d] (got %d)", ROOM_MAX_S, S);
  if (M < 1 || M > ROOM_MAX_M) return fail(MISONET_EINVAL, "M must be in [1, %d] (got %d)", ROOM_MAX_M, M);
  if (Lh < 1 || Lh > ROOM_MAX_LH) return fail(MISONET_EINVAL, "Lh must be in [1, %d] (got %d)", ROOM_MAX_LH, Lh);
  return MISONET_OK;
}

int misonet_room_tile(void) { return room_tile(); }

long long misonet_room_rir_len(int B, int S, int M, int Lh) {
  if (B < 1 || B > ROOM_MAX_B || S < 1 || S > ROOM_MAX_S || M < 1 || M > ROOM_MAX_M || Lh < 1 || Lh > ROOM_MAX_LH) return -1;
  return (long long)B * S * M * Lh;
}

long long misonet_room_mix_len(long long L, int Lh) {
  if (L < 1 || L > ROOM_MAX_L || Lh < 1 || Lh > ROOM_MAX_LH) return -1;
  return L + Lh - 1;
}

int misonet_room_rir(const double* room_dev, const double* beta_dev, const double* src_dev, const double* mic_dev, int B, int S,
                     int M, double fs, double c, int Lh, int max_order, double* rir_dev, int* fail_dev, misonet_stream stream) {
  { int r = room_geometry(B, S, M, Lh); if (r) return r; }
  if (!(fs > 0.0) || !std::isfinite(fs)) return fail(MISONET_EINVAL, "fs must be finite and > 0 (got %g)", fs);
  if (!(c > 0.0) || !std::isfinite(c)) return fail(MISONET_EINVAL, "c must be finite and > 0 (got %g)", c);
  if (max_order < -1) return fail(MISONET_EINVAL, "max_order must be -1 (no limit) or >= 0 (got %d)", max_order);
  if (!room_dev || !beta_dev || !src_dev || !mic_dev || !rir_dev || !fail_dev) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_room_rir(room_dev, beta_dev, src_dev, mic_dev, B, S, M, fs, c, Lh, max_order, rir_dev, fail_dev,
                         reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_room_mix(const float* src_dev, long long src_sb, long long src_ss, long long src_st, const double* rir_dev,
                     const int* split_dev, int B, int S, int M, long long L, int Lh, long long Lo, float* images_dev,
                     float* early_dev, float* mix_dev, misonet_stream stream) {
  { int r = room_geometry(B, S, M, Lh); if (r) return r; }
  if (L < 1 || L > ROOM_MAX_L) return fail(MISONET_EINVAL, "L must be in [1, 2^24] (got %lld)", L);
  if (Lo < 1 || Lo > L + Lh - 1) return fail(MISONET_EINVAL, "Lo must be in [1, L + Lh - 1] = [1, %lld] (got %lld)", L + Lh - 1, Lo);
  if (src_sb < 0 || src_ss < 0 || src_st < 1)
    return fail(MISONET_EINVAL, "source strides must not be negative and the sample stride must be positive");
  if (((Lo + room_tile() - 1) / room_tile()) * M * B * room_tile() >= (1LL << 32))
    return fail(MISONET_EINVAL, "B x M x Lo = %d x %d x %lld is more than one call takes (2^32 output samples)", B, M, Lo);
  if (!src_dev || !rir_dev || !images_dev) return fail(MISONET_EINVAL, "null argument");
  const long long xs[3] = {src_sb, src_ss, src_st};
  HIPCHK(launch_room_mix(src_dev, xs, rir_dev, split_dev, B, S, M, (int)L, Lh, (int)Lo, images_dev, early_dev, mix_dev,
                         reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- source localisation (doa.hip) ----------------------------------------------------------------------------------------------
int misonet_doa_opts_default(misonet_doa_opts* o) {
  if (!o) return fail(MISONET_EINVAL, "null argument");
  o->kind = DOA_SRP_PHAT; o->num_src = 1; o->block = 0; o->hop = 0; o->f_lo = 0; o->f_hi = -1; o->min_sep = 0.0;
  return MISONET_OK;
}

int misonet_doa_tile(void) { return doa_tile(); }
int misonet_doa_bin_chunk(void) { return doa_bin_chunk(); }

int misonet_doa_blocks(int T, int block, int hop) {
  if (T < 1 || block < 0 || hop < 0 || block > T) return -1;
  if (block == 0) return 1;
  return 1 + (T - block) / (hop ? hop : block);
}

// every limit of the call; *N, *f_hi: the resolved block count and last bin.  quiet: the size function sets no message
static int doa_check(int B, int K, int F, int M, int T, int D, const misonet_doa_opts* o, int* N, int* f_hi, bool quiet) {
#define DOA_BAD(...) return quiet ? MISONET_EINVAL : fail(MISONET_EINVAL, __VA_ARGS__)
  if (!o) DOA_BAD("null localisation options");
  if (B < 1 || F < 1 || T < 1) DOA_BAD("B, F and T must be positive (got %d, %d, %d)", B, F, T);
  if (M < 2 || M > 8) DOA_BAD("M must be in [2, 8] (got %d)", M);
  if (K < 1 || K > DOA_MAX_K) DOA_BAD("K must be in [1, %d] (got %d)", DOA_MAX_K, K);
  if (D < 1 || D > DOA_MAX_D) DOA_BAD("D must be in [1, %d] (got %d)", DOA_MAX_D, D);
  if (o->kind != DOA_SRP && o->kind != DOA_SRP_PHAT && o->kind != DOA_MUSIC) DOA_BAD("kind %d: 0 srp, 1 srp_phat, 2 music", o->kind);
  if (o->num_src < 1 || o->num_src > DOA_MAX_S || o->num_src > D)
    DOA_BAD("num_src must be in [1, min(%d, D)] (got %d, D %d)", DOA_MAX_S, o->num_src, D);
  if (o->kind == DOA_MUSIC && o->num_src > M - 1) DOA_BAD("music needs num_src <= M - 1 = %d (got %d)", M - 1, o->num_src);
  if (o->block < 0 || o->hop < 0 || o->block > T) DOA_BAD("block must be in [0, T] and hop >= 0 (got block %d, hop %d, T %d)", o->block, o->hop, T);
  const int fh = o->f_hi == -1 ? F - 1 : o->f_hi;
  if (o->f_lo < 0 || o->f_lo > fh || fh >= F) DOA_BAD("0 <= f_lo <= f_hi < F does not hold (got %d, %d, F %d)", o->f_lo, o->f_hi, F);
  if (!(o->min_sep >= 0.0) || !std::isfinite(o->min_sep)) DOA_BAD("min_sep must be finite and >= 0 (got %g)", o->min_sep);
  const int n = misonet_doa_blocks(T, o->block, o->hop);
  if ((long long)B * K * n * D >= (1LL << 31)) DOA_BAD("B K N D must stay under 2^31 (got B %d, K %d, N %d, D %d)", B, K, n, D);
  // the launch grids: one 64-thread workgroup per (b, n, f), one doa_tile()-thread workgroup per (b, k, n, tile), under 2^32 threads
  const long long tiles = (D + doa_tile() - 1) / doa_tile();
  if ((long long)B * n * F * 64 >= (1LL << 32) || (long long)B * K * n * tiles * doa_tile() >= (1LL << 32))
    DOA_BAD("B N F = %lld bins or B K N ceil(D / %d) = %lld tiles are more than one call takes (2^26 bins, 2^32 / %d tiles)",
            (long long)B * n * F, doa_tile(), (long long)B * K * n * tiles, doa_tile());
#undef DOA_BAD
  *N = n;
  *f_hi = fh;
  return MISONET_OK;
}

long long misonet_doa_workspace_bytes(int B, int K, int F, int M, int T, int D, const misonet_doa_opts* opts) {
  int N = 0, fh = 0;
  if (doa_check(B, K, F, M, T, D, opts, &N, &fh, true)) return -1;
  return doa_ws_bytes(B, K, N, F, M);
}

int misonet_doa(const void* mix, const float* weight, const double* tau, int Bg, const double* pts, int B, int K, int F, int M,
                int T, int D, double fs, const misonet_doa_opts* opts, double* q_out, int* peak_out, double* value_out,
                int* fail_out, void* ws, long long ws_bytes, misonet_stream stream) {
  int N = 0, fh = 0;
  { int r = doa_check(B, K, F, M, T, D, opts, &N, &fh, false); if (r) return r; }
  if (Bg != 1 && Bg != B) return fail(MISONET_EINVAL, "the delay table's batch must be 1 or B = %d (got %d)", B, Bg);
  if (!(fs > 0.0) || !std::isfinite(fs)) return fail(MISONET_EINVAL, "fs must be finite and > 0 (got %g)", fs);
  if (!weight && K != 1) return fail(MISONET_EINVAL, "without weights K must be 1 (got %d)", K);
  if (!mix || !tau || !pts || !q_out || !peak_out || !value_out || !fail_out || !ws) return fail(MISONET_EINVAL, "null argument");
  if (ws_bytes < doa_ws_bytes(B, K, N, F, M)) return fail(MISONET_ENOMEM, "workspace too small");
  DoaArgs a;
  a.mix = reinterpret_cast<const float2*>(mix); a.weight = weight; a.tau = tau; a.pts = pts;
  a.Bg = Bg; a.B = B; a.K = K; a.F = F; a.M = M; a.T = T; a.D = D;
  a.fs = fs;
  a.kind = opts->kind; a.S = opts->num_src;
  a.block = opts->block ? opts->block : T;
  a.hop = opts->block ? (opts->hop ? opts->hop : opts->block) : T;
  a.N = N; a.f_lo = opts->f_lo; a.f_hi = fh;
  a.min_sep = opts->min_sep;
  a.q = q_out; a.peak = peak_out; a.value = value_out; a.fail = fail_out;
  HIPCHK(launch_doa(a, ws, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_doa_debug(const void* ws, int B, int K, int F, int M, int T, int D, const misonet_doa_opts* opts, void* c_c128_dev,
                      int* used_dev, int* fail_dev, misonet_stream stream) {
  int N = 0, fh = 0;
  { int r = doa_check(B, K, F, M, T, D, opts, &N, &fh, false); if (r) return r; }
  if (!ws) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(launch_doa_debug(ws, B, K, N, F, M, c_c128_dev, used_dev, fail_dev, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

long long misonet_pit_scratch_bytes(int B, int S, int F) {
  if (B <= 0 || S <= 0 || F <= 0) return -1;
  return (long long)B * S * S * (F + 1) * (long long)sizeof(double);
}

int misonet_pit_select(const void* anchor, const void* cand, int B, int S, int T, int F, int* sel, double* dist,
                       long long dist_bytes, misonet_stream stream) {
  if (!anchor || !cand || !sel || !dist) return fail(MISONET_EINVAL, "null argument (dist is required: B*S*S*(F+1) doubles)");
  if (S < 1 || S > 4) return fail(MISONET_EINVAL, "PIT alignment enumerates S! permutations: 1 <= num_spks <= 4 (got %d)", S);
  if (B <= 0 || T <= 0 || F <= 0) return fail(MISONET_EINVAL, "B, T, F must be positive");
  if (dist_bytes < misonet_pit_scratch_bytes(B, S, F))
    return fail(MISONET_ENOMEM, "dist scratch %lld < %lld bytes (B*S*S*(F+1) doubles)", dist_bytes, misonet_pit_scratch_bytes(B, S, F));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float* a = reinterpret_cast<const float*>(anchor);
  const float* c = reinterpret_cast<const float*>(cand);
  PitArgs p;
  // [B,S,T,F] complex64: element (b, f, spk, t) at ((b*S + spk)*T + t)*F + f
  p.a = {a, a + 1, 2LL * S * T * F, 2, 2LL * T * F, 2 * F};
  p.b = {c, c + 1, 2LL * S * T * F, 2, 2LL * T * F, 2 * F};
  p.B = B; p.F = F; p.T = T;
  double* part = dist + (long long)B * S * S;          // per-bin partials [B][F][S][S] behind the result
  HIPCHK(launch_pit_dist_k(p, S, 1, part, s));
  HIPCHK(launch_pit_pick(part, F, S, B, dist, sel, s));
  return MISONET_OK;
}

// ---- continuous separation: speaker tracking across overlapping windows + cross-fade stitch (css.hip) -------------
long long misonet_css_scratch_bytes(int K, int S, int F) {
  if (K <= 0 || S <= 0 || F <= 0) return -1;
  return (long long)(K - 1) * S * S * (F + 1) * (long long)sizeof(double);
}

int misonet_css_align(const void* est, int K, int S, int T, int F, int hop_frames, const int* perm0, int* perm,
                      double* dist, long long dist_bytes, misonet_stream stream) {
  if (!est || !perm) return fail(MISONET_EINVAL, "null argument");
  if (S < 1 || S > 4) return fail(MISONET_EINVAL, "the alignment enumerates S! permutations: 1 <= S <= 4 (got %d)", S);
  if (F != 129) return fail(MISONET_EINVAL, "F must be 129 (got %d)", F);
  if (K < 1 || K - 1 > 65535) return fail(MISONET_EINVAL, "K must be in [1, 65536] (got %d)", K);
  if (hop_frames <= 0 || T - hop_frames < 5)
    return fail(MISONET_EINVAL, "hop_frames must be positive and leave an overlap of at least 5 frames (T %d, hop %d)", T,
                hop_frames);
  if (K > 1 && !dist) return fail(MISONET_EINVAL, "null argument (dist is required for K > 1: (K-1)*S*S*(F+1) doubles)");
  if (dist_bytes < misonet_css_scratch_bytes(K, S, F))
    return fail(MISONET_ENOMEM, "dist scratch %lld < %lld bytes ((K-1)*S*S*(F+1) doubles)", dist_bytes,
                misonet_css_scratch_bytes(K, S, F));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (K > 1) {
    // est complex64 [K,S,T,F]: element (k, f, spk, t) at ((k*S + spk)*T + t)*F + f.  Item b = k - 1 of the distance launch:
    // anchor = window k - 1 from frame hop_frames on, candidate = window k from frame 0, over the T - hop_frames shared frames
    const float* e = reinterpret_cast<const float*>(est);
    const long long win = 2LL * S * T * F;
    const float* a = e + 2LL * hop_frames * F;
    const float* c = e + win;
    PitArgs p;
    p.a = {a, a + 1, win, 2, 2LL * T * F, 2 * F};
    p.b = {c, c + 1, win, 2, 2LL * T * F, 2 * F};
    p.B = K - 1; p.F = F; p.T = T - hop_frames;
    double* part = dist + (long long)(K - 1) * S * S;                // per-bin partials [K-1][F][S][S] behind D
    HIPCHK(launch_pit_dist_k(p, S, 1, part, s));
    HIPCHK(launch_pit_pick(part, F, S, K - 1, dist, perm + S, s));   // L_k -> row k of perm, composed in place below
  }
  HIPCHK(launch_css_chain(perm0, perm, K, S, s));
  return MISONET_OK;
}

int misonet_css_stitch(const float* y, const int* perm, int K, int S, int W, int hop, int first, long long n_out,
                       short* out_i16, float* out_f32, misonet_stream stream) {
  if (!y || !perm || (!out_i16 && !out_f32)) return fail(MISONET_EINVAL, "null argument");
  if (S < 1 || S > 4) return fail(MISONET_EINVAL, "S must be in [1, 4] (got %d)", S);
  if (K < 1) return fail(MISONET_EINVAL, "K must be positive (got %d)", K);
  if (W <= 0 || hop <= 0 || 2LL * hop < W || hop > W - 256)
    return fail(MISONET_EINVAL, "hop %d outside [W/2, W-256] for W = %d", hop, W);
  const long long base = first ? 0 : hop;
  const long long cap = (long long)(K - 1) * hop + W - base;
  if (n_out < 0 || n_out > cap) return fail(MISONET_EINVAL, "n_out %lld outside [0, %lld]", n_out, cap);
  if (n_out == 0) return MISONET_OK;
  HIPCHK(launch_css_stitch(y, perm, K, S, W, hop, base, n_out, out_i16, out_f32, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

}  // extern "C"
