// C ABI of the STFT front-end (include/misonet.h): misonet_stft*, misonet_istft, misonet_frontend_init, and the twiddle tables of
// stft.hip on every device that uses them; the resampler in front of it, misonet_resample* (resample.hip), and its tap tables.
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

}  // extern "C"
