// C ABI of the STFT front-end (include/misonet.h): misonet_stft*, misonet_istft, misonet_frontend_init, the streaming forms
// misonet_stft_stream* / misonet_istft_stream*, and the twiddle tables of stft.hip on every device that uses them; the resampler in front of it, misonet_resample* (resample.hip), its streaming form misonet_resample_stream* (resample_stream.hip), and their tap tables.
// Host code only.
#include "api_common.hpp"

#include <map>
#include <tuple>

using namespace mn;

// twiddle table + the > 64 KB dynamic-LDS attribute of stft_pack_k, per device (the table lives in the memory of the
// device that was current when it was first needed)
static DevTable<float> g_twid, g_itwid;
// Both tables of the CURRENT device, built if this is the first use there (hipMalloc + synchronous copy + kernel attributes: not
// inside a stream capture; include/misonet.h).  Idempotent, thread-safe.
static int frontend_tables(const float** tw, const float** itw) {
  int r = g_twid.get(tw, [](float** p) -> int {
    std::vector<float> t((size_t)stft_twiddle_count());
    stft_build_twiddles(t.data());
    if (const int rc = dev_upload(t, p)) return rc;
    HIPCHK(stft_init());
    return MISONET_OK;
  });
  if (r) return r;
  return g_itwid.get(itw, [](float** p) -> int {
    std::vector<float> t((size_t)istft_twiddle_count());
    istft_build_twiddles(t.data());
    if (const int rc = dev_upload(t, p)) return rc;
    HIPCHK(istft_init());
    HIPCHK(stft_stream_init());
    return MISONET_OK;
  });
}
int mn::get_twiddles(const float** out) {
  const float* itw;
  return frontend_tables(out, &itw);
}

// ---- the resampler's taps: one table per (device, p, q), built at the first use there and kept ------------------------------
static std::mutex g_rs_mu;
static std::map<std::tuple<int, int, int>, double*> g_rs_taps;
static int resample_table(int p, int q, const double** out) {
  const std::tuple<int, int, int> key(cur_dev(), p, q);
  std::lock_guard<std::mutex> lk(g_rs_mu);
  auto it = g_rs_taps.find(key);
  if (it == g_rs_taps.end()) {
    std::vector<double> t((size_t)(2 * resample_half_len(p, q) + 1));
    resample_build_taps(p, q, t.data());
    double* d = nullptr;
    if (const int rc = dev_upload(t, &d)) return rc;
    it = g_rs_taps.emplace(key, d).first;
  }
  *out = it->second;
  return MISONET_OK;
}
static int resample_rates(int fs_in, int fs_out, int* p, int* q) {
  if (!resample_ratio(fs_in, fs_out, p, q))
    return fail(MISONET_EINVAL, "fs_in and fs_out must be positive with max(p, q) <= %d for p / q = fs_out / fs_in in lowest "
                "terms (got %d -> %d)", RS_MAX_RATE, fs_in, fs_out);
  return MISONET_OK;
}
constexpr long long RS_MAX_N = 1LL << 28;

extern "C" {

// ---- polyphase resampler (resample.hip) --------------------------------------------------------------------------------------
int misonet_resample_ratio(int fs_in, int fs_out, int* p, int* q) {
  int pp, qq;
  if (const int rc = resample_rates(fs_in, fs_out, &pp, &qq)) return rc;
  if (p) *p = pp;
  if (q) *q = qq;
  return MISONET_OK;
}

long long misonet_resampled_len(long long n, int fs_in, int fs_out) {
  int p, q;
  if (n < 1 || n > RS_MAX_N || !resample_ratio(fs_in, fs_out, &p, &q)) return -1;
  return resample_len(n, p, q);
}

int misonet_resample_tile(void) { return resample_tile(); }

int misonet_resample_taps(int fs_in, int fs_out, double* out, int cap) {
  int p, q;
  if (const int rc = resample_rates(fs_in, fs_out, &p, &q)) return rc;
  const int nt = 2 * resample_half_len(p, q) + 1;
  if (out) {
    if (cap < nt) return fail(MISONET_EINVAL, "cap %d < %d taps", cap, nt);
    resample_build_taps(p, q, out);
  }
  return nt;
}

int misonet_resample(const void* src_dev, int src_kind, long long src_sb, long long src_sc, long long src_st, int B, int M,
                     long long n, const int* n_valid_dev, int fs_in, int fs_out, void* dst_dev, int dst_kind, long long dst_sb,
                     long long dst_sc, long long dst_st, misonet_stream stream) {
  int p, q;
  if (const int rc = resample_rates(fs_in, fs_out, &p, &q)) return rc;
  if ((src_kind != 0 && src_kind != 1) || (dst_kind != 0 && dst_kind != 1))
    return fail(MISONET_EINVAL, "src_kind and dst_kind must be 0 (float32) or 1 (int16) (got %d, %d)", src_kind, dst_kind);
  if (B < 1 || B > 65535) return fail(MISONET_EINVAL, "B must be in [1, 65535] (got %d)", B);
  if (M < 1 || M > RS_MAX_CH) return fail(MISONET_EINVAL, "M must be in [1, %d] (got %d)", RS_MAX_CH, M);
  if (n < 1 || n > RS_MAX_N) return fail(MISONET_EINVAL, "n must be in [1, 2^28] (got %lld)", n);
  if (src_sb < 0 || src_sc < 0 || src_st < 1)
    return fail(MISONET_EINVAL, "source strides must not be negative and the sample stride must be positive");
  if (dst_st < 1 || (M > 1 && dst_sc < 1) || (B > 1 && dst_sb < 1) || dst_sc < 0 || dst_sb < 0)
    return fail(MISONET_EINVAL, "destination strides must be positive along every axis longer than 1");
  if (!src_dev || !dst_dev) return fail(MISONET_EINVAL, "null argument");
  const double* taps;
  if (const int rc = resample_table(p, q, &taps)) return rc;
  const long long ss[3] = {src_sb, src_sc, src_st}, ds[3] = {dst_sb, dst_sc, dst_st};
  HIPCHK(launch_resample(src_dev, src_kind, ss, B, M, n, n_valid_dev, p, q, taps, dst_dev, dst_kind, ds,
                         reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- streaming polyphase resampler (resample_stream.hip; ABI 660) -----------------------------------------
constexpr long long RSS_MAX_SEEN = 1LL << 50;
static bool rss_counts_ok(long long seen, long long add, int flush) {
  return seen >= 0 && seen <= RSS_MAX_SEEN && add >= 0 && add <= RS_MAX_N && (add >= 1 || flush);
}

long long misonet_resample_stream_carry(long long fs_in, long long fs_out) {
  int p, q;
  if (!resample_ratio(fs_in, fs_out, &p, &q)) return -1;
  return resample_stream_carry(p, q);
}

long long misonet_resample_stream_state_bytes(int B, int M, long long fs_in, long long fs_out) {
  int p, q;
  if (B < 1 || B > 65535 || M < 1 || M > RS_MAX_CH || !resample_ratio(fs_in, fs_out, &p, &q)) return -1;
  return (long long)B * M * resample_stream_carry(p, q) * (long long)sizeof(float);
}

long long misonet_resample_stream_outputs(long long n_seen, long long n_new, int flush, long long fs_in, long long fs_out) {
  int p, q;
  if (!rss_counts_ok(n_seen, n_new, flush) || !resample_ratio(fs_in, fs_out, &p, &q)) return -1;
  const long long E = flush ? resample_len(n_seen + n_new, p, q) : resample_stream_emitted(n_seen + n_new, p, q);
  return E - resample_stream_emitted(n_seen, p, q);
}

int misonet_resample_stream_tile(void) { return resample_stream_tile(); }

static int rss_shape(int B, int M, long long fs_in, long long fs_out, long long* nb) {
  int p, q;
  if (!resample_ratio(fs_in, fs_out, &p, &q))
    return fail(MISONET_EINVAL, "fs_in and fs_out must be positive with max(p, q) <= %d for p / q = fs_out / fs_in in lowest "
                "terms (got %lld -> %lld)", RS_MAX_RATE, fs_in, fs_out);
  if (B < 1 || B > 65535) return fail(MISONET_EINVAL, "B must be in [1, 65535] (got %d)", B);
  if (M < 1 || M > RS_MAX_CH) return fail(MISONET_EINVAL, "M must be in [1, %d] (got %d)", RS_MAX_CH, M);
  *nb = misonet_resample_stream_state_bytes(B, M, fs_in, fs_out);
  return MISONET_OK;
}

int misonet_resample_stream_reset(void* state_dev, int B, int M, long long fs_in, long long fs_out, misonet_stream stream) {
  long long nb;
  if (const int rc = rss_shape(B, M, fs_in, fs_out, &nb)) return rc;
  if (nb == 0) return MISONET_OK;                                       // 1 / 1 carries nothing
  if (!state_dev) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(hipMemsetAsync(state_dev, 0, (size_t)nb, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_resample_stream(const void* src_dev, int src_i16, long long src_sb, long long src_sc, long long src_st, int B, int M,
                            long long n_new, long long n_seen, int flush, long long fs_in, long long fs_out, void* dst_dev,
                            int dst_i16, long long dst_sb, long long dst_sc, long long dst_st, void* state_dev,
                            long long state_bytes, misonet_stream stream) {
  long long nb;
  if (const int rc = rss_shape(B, M, fs_in, fs_out, &nb)) return rc;
  if ((src_i16 != 0 && src_i16 != 1) || (dst_i16 != 0 && dst_i16 != 1))
    return fail(MISONET_EINVAL, "src_i16 and dst_i16 must be 0 (float32) or 1 (int16) (got %d, %d)", src_i16, dst_i16);
  const long long n_out = misonet_resample_stream_outputs(n_seen, n_new, flush, fs_in, fs_out);
  if (n_out < 0)
    return fail(MISONET_EINVAL, "n_seen must be in [0, 2^50] and n_new in [%d, 2^28] (got %lld, %lld, flush %d)", flush ? 0 : 1,
                n_seen, n_new, flush);
  if (src_sb < 0 || src_sc < 0 || src_st < 1)
    return fail(MISONET_EINVAL, "source strides must not be negative and the sample stride must be positive");
  if (dst_st < 1 || (M > 1 && dst_sc < 1) || (B > 1 && dst_sb < 1) || dst_sc < 0 || dst_sb < 0)
    return fail(MISONET_EINVAL, "destination strides must be positive along every axis longer than 1");
  if ((nb > 0 && !state_dev) || (n_new > 0 && !src_dev) || (n_out > 0 && !dst_dev)) return fail(MISONET_EINVAL, "null argument");
  if (state_bytes < nb) return fail(MISONET_ENOMEM, "state too small: %lld < %lld bytes", state_bytes, nb);
  int p, q;
  resample_ratio(fs_in, fs_out, &p, &q);
  const double* taps;
  if (const int rc = resample_table(p, q, &taps)) return rc;
  // the first output of the call against the block's first sample, in tap units: all a launch knows of n_seen
  const long long D = resample_stream_emitted(n_seen, p, q) * q - n_seen * p;
  const long long ss[3] = {src_sb, src_sc, src_st}, ds[3] = {dst_sb, dst_sc, dst_st};
  HIPCHK(launch_resample_stream(src_dev, src_i16, ss, B, M, n_new, D, n_out, !flush, p, q, taps, dst_dev, dst_i16, ds,
                                reinterpret_cast<float*>(state_dev), reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// misonet_net_commit and misonet_pipeline_create call it, so every path that runs a network has the tables before its first
// asynchronous call -- a HIP graph may capture misonet_pipeline_run_wav / misonet_istft as the first call of a process.  A
// stand-alone misonet_stft / misonet_istft without any committed network on this device builds them on first use.
int misonet_frontend_init(void) {
  const float *tw, *itw;
  return frontend_tables(&tw, &itw);
}

int misonet_istft(const void* spec_dev, int N, int T, void* out_i16_dev, float* out_f32_dev, misonet_stream stream) {
  if (!spec_dev || (!out_i16_dev && !out_f32_dev)) return fail(MISONET_EINVAL, "null argument");
  if (N <= 0 || T < 2) return fail(MISONET_EINVAL, "N must be positive and T >= 2 (got %d, %d)", N, T);
  const float *tw, *itw;
  int r = frontend_tables(&tw, &itw);
  if (r) return r;
  HIPCHK(launch_istft(spec_dev, N, T, itw, reinterpret_cast<short*>(out_i16_dev), out_f32_dev,
                      reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_stft_frames(int n_samples) { return n_samples > 0 ? n_samples / 64 + 1 : -1; }

long long misonet_stft_workspace_bytes(int B, int M, int n_samples) {
  const int T = misonet_stft_frames(n_samples);
  if (B <= 0 || M <= 0 || T <= 0) return -1;
  return (long long)B * 2 * M * 129 * frames_pitch(T) * 4;
}

int misonet_stft(const float* wav_dev, int B, int n_samples, int M, void* out_c64, void* ws, long long ws_bytes,
                 misonet_stream stream) {
  if (!wav_dev || !out_c64 || !ws) return fail(MISONET_EINVAL, "null argument");
  if (B <= 0 || M <= 0 || M > 64 || n_samples <= 0) return fail(MISONET_EINVAL, "bad B / M / n_samples");
  if (ws_bytes < misonet_stft_workspace_bytes(B, M, n_samples)) return fail(MISONET_ENOMEM, "workspace too small");
  const int T = misonet_stft_frames(n_samples), Tp = frames_pitch(T), F = 129;
  const float* tw;
  int r = get_twiddles(&tw);
  if (r) return r;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* planar = reinterpret_cast<float*>(ws);
  const long long bs = 2LL * M * F * Tp;
  HIPCHK(launch_stft_pack(wav_dev, B, n_samples, M, T, tw, planar, bs, Tp, F, 0, M, 1, s));
  HIPCHK(launch_unpack(planar, bs, Tp, M, T, F, reinterpret_cast<float2*>(out_c64), B, nullptr, s));
  return MISONET_OK;
}

// ---- streaming STFT / iSTFT: waveform blocks in, frames out; frames in, hops out (ABI 650) ---------------
constexpr long long SS_MAX_N = 1LL << 28, SS_MAX_T = 1LL << 22;
static long long ss_emitted(long long N) { return N / 64 - 1 > 0 ? N / 64 - 1 : 0; }        // e(N)
static long long iss_emitted(long long Tc) { return Tc - 2 > 0 ? Tc - 2 : 0; }              // g(Tc)
static bool ss_counts_ok(long long seen, long long add, int flush, long long cap) {
  return seen >= 0 && add >= 0 && add <= cap && (add >= 1 || flush) && seen <= (1LL << 62);
}

long long misonet_stft_stream_state_bytes(int B, int M) {
  if (B < 1 || B > 65535 || M < 1 || M > 64) return -1;
  return stft_stream_state_bytes((long long)B * M);
}

long long misonet_stft_stream_frames(long long n_seen, long long n_new, int flush) {
  if (!ss_counts_ok(n_seen, n_new, flush, SS_MAX_N)) return -1;
  const long long E = flush ? (n_seen + n_new) / 64 + 1 : ss_emitted(n_seen + n_new);
  return E - ss_emitted(n_seen);
}

int misonet_stft_stream_reset(void* state_dev, int B, int M, misonet_stream stream) {
  const long long nb = misonet_stft_stream_state_bytes(B, M);
  if (nb < 0) return fail(MISONET_EINVAL, "B must be in [1, 65535] and M in [1, 64] (got %d, %d)", B, M);
  if (!state_dev) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(hipMemsetAsync(state_dev, 0, (size_t)nb, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_stft_stream(const float* wav_dev, int B, long long n_new, int M, long long n_seen, int flush, void* out_c64_dev,
                        void* state_dev, long long state_bytes, misonet_stream stream) {
  const long long nb = misonet_stft_stream_state_bytes(B, M);
  if (nb < 0) return fail(MISONET_EINVAL, "B must be in [1, 65535] and M in [1, 64] (got %d, %d)", B, M);
  const long long Tn = misonet_stft_stream_frames(n_seen, n_new, flush);
  if (Tn < 0)
    return fail(MISONET_EINVAL, "n_seen must be >= 0 and n_new in [%d, 2^28] (got %lld, %lld, flush %d)", flush ? 0 : 1, n_seen,
                n_new, flush);
  if (!state_dev || (n_new > 0 && !wav_dev) || (Tn > 0 && !out_c64_dev)) return fail(MISONET_EINVAL, "null argument");
  if (state_bytes < nb) return fail(MISONET_ENOMEM, "state too small: %lld < %lld bytes", state_bytes, nb);
  const float* tw;
  if (const int r = get_twiddles(&tw)) return r;
  // the first frame of the call starts 64 e(n_seen) - 128 - n_seen samples from the block's first one: -128 - n_seen before the
  // stream has 128 samples, -192 - n_seen mod 64 ever after
  const int off0 = (int)(64 * ss_emitted(n_seen) - 128 - n_seen);
  HIPCHK(launch_stft_stream(wav_dev, B, (int)n_new, M, (int)Tn, off0, !flush, tw, reinterpret_cast<float2*>(out_c64_dev),
                            reinterpret_cast<float*>(state_dev), reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

long long misonet_istft_stream_state_bytes(int R) {
  if (R < 1 || R > 65535) return -1;
  return istft_stream_state_bytes(R);
}

long long misonet_istft_stream_hops(long long t_seen, long long t_new, int flush) {
  if (!ss_counts_ok(t_seen, t_new, flush, SS_MAX_T)) return -1;
  const long long Tt = t_seen + t_new;
  const long long G = flush ? (Tt - 1 > 0 ? Tt - 1 : 0) : iss_emitted(Tt);
  return G - iss_emitted(t_seen);
}

int misonet_istft_stream_reset(void* state_dev, int R, misonet_stream stream) {
  const long long nb = misonet_istft_stream_state_bytes(R);
  if (nb < 0) return fail(MISONET_EINVAL, "R must be in [1, 65535] (got %d)", R);
  if (!state_dev) return fail(MISONET_EINVAL, "null argument");
  HIPCHK(hipMemsetAsync(state_dev, 0, (size_t)nb, reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_istft_stream(const void* spec_dev, int R, long long t_new, long long t_seen, int flush, void* out_i16_dev,
                         float* out_f32_dev, void* state_dev, long long state_bytes, misonet_stream stream) {
  const long long nb = misonet_istft_stream_state_bytes(R);
  if (nb < 0) return fail(MISONET_EINVAL, "R must be in [1, 65535] (got %d)", R);
  const long long H = misonet_istft_stream_hops(t_seen, t_new, flush);
  if (H < 0)
    return fail(MISONET_EINVAL, "t_seen must be >= 0 and t_new in [%d, 2^22] (got %lld, %lld, flush %d)", flush ? 0 : 1, t_seen,
                t_new, flush);
  if (!state_dev || (t_new > 0 && !spec_dev) || (H > 0 && !out_i16_dev && !out_f32_dev))
    return fail(MISONET_EINVAL, "null argument");
  if (state_bytes < nb) return fail(MISONET_ENOMEM, "state too small: %lld < %lld bytes", state_bytes, nb);
  const float *tw, *itw;
  if (const int r = frontend_tables(&tw, &itw)) return r;
  // hop 0 of the call needs the frames g(t_seen) - 1 .. + 2: counted from the first new frame that is -3 once two frames have
  // been seen; min(t_seen, 3) of the carried frames exist
  const int fr0 = (int)(iss_emitted(t_seen) - 1 - t_seen), lead = (int)(t_seen < 3 ? t_seen : 3);
  HIPCHK(launch_istft_stream(spec_dev, R, (int)t_new, lead, fr0, (int)H, !flush && t_new > 0, itw,
                             reinterpret_cast<short*>(out_i16_dev), out_f32_dev, state_dev,
                             reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

}  // extern "C"
