// C ABI of the STFT front-end (include/misonet.h): misonet_stft*, misonet_istft, misonet_frontend_init, and the twiddle tables of
// stft.hip on every device that uses them.  Host code only.
#include "api_common.hpp"

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

extern "C" {

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
