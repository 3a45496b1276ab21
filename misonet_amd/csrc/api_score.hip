// C ABI of the scoring against clean references (include/misonet.h): misonet_score_* (score.hip), BSS-eval misonet_bss_*
// (bss.hip), STOI / ESTOI misonet_stoi_* (stoi.hip), cepstral distance / LLR / fwSegSNR misonet_reverb_* (reverb.hip), SRMR misonet_srmr_* (srmr.hip) and the
// STOI, reverb and SRMR tables of every device that uses them.  Host code only.
#include "api_common.hpp"

using namespace mn;

// ---- checks the scorers share --------------------------------------------------------------------------------------------
// the strided views of estimates and references: (item, source, sample) strides, or frame strides for the spectral score (`unit`)
static int view_strides(long long est_sb, long long est_ss, long long est_st, long long ref_sb, long long ref_ss,
                        long long ref_st, const char* unit, bool mix_bad = false) {
  if (est_sb < 0 || est_ss < 0 || est_st < 1 || ref_sb < 0 || ref_ss < 0 || ref_st < 1 || mix_bad)
    return fail(MISONET_EINVAL, "strides must not be negative and the %s strides must be positive", unit);
  return MISONET_OK;
}
// the views of a waveform scorer (sig_view.hpp) from the arguments of its entry point, strides checked: estimates (float32, or
// int16 where i16), references and the mixture, one signal per item; a call without references or without a mixture passes
// nullptr there, with the strides {0, 0, 1} and {0, 1}
struct ScoreViews { SigView est, ref, mix; };
static int score_views(ScoreViews* v, const void* est, int i16, long long est_sb, long long est_ss, long long est_st,
                       const float* ref, long long ref_sb, long long ref_ss, long long ref_st, const float* mix = nullptr,
                       long long mix_sb = 0, long long mix_st = 1) {
  if (const int rc = view_strides(est_sb, est_ss, est_st, ref_sb, ref_ss, ref_st, "sample", mix && (mix_sb < 0 || mix_st < 1)))
    return rc;
  *v = {{est, est_sb, est_ss, est_st, i16 != 0}, {ref, ref_sb, ref_ss, ref_st, 0}, {mix, mix ? mix_sb : 0, 0, mix ? mix_st : 1, 0}};
  return MISONET_OK;
}
// the constant table of a scorer on the current device (window, twiddles, filter taps and the like), built on the host and
// uploaded at the first use there: that one call allocates and copies synchronously; every later call only queues kernels
static int score_table(DevTable<double>& tab, int count, void (*build)(double*), const double** out) {
  return tab.get(out, [&](double** p) {
    std::vector<double> t((size_t)count);
    build(t.data());
    return dev_upload(t, p);
  });
}
// `sizing`: the call that gives `need`, as the message names it
static int scratch_fits(long long scratch_bytes, long long need, const char* sizing) {
  if (scratch_bytes < need) return fail(MISONET_ENOMEM, "scratch %lld < %lld bytes (%s)", scratch_bytes, need, sizing);
  return MISONET_OK;
}
// estimates, references and items of BSS-eval and STOI (misonet_score_* take the mixture as a fifth estimate: score_ranges)
static int erb_ranges(int B, int E, int R) {
  if (E < 1 || E > 4) return fail(MISONET_EINVAL, "E must be in [1, 4] (got %d)", E);
  if (R < 1 || R > 4) return fail(MISONET_EINVAL, "R must be in [1, 4] (got %d)", R);
  if (B < 1 || B > 4096) return fail(MISONET_EINVAL, "B must be in [1, 4096] (got %d)", B);
  return MISONET_OK;
}

extern "C" {

// ---- scores against clean references (score.hip) --------------------------------------------------------------------
// One size serves both entry points: the wave partials [B][ceil(n / 4096)][2E + 2R + E R] and the per-bin partials
// [B][F][E][R] (F <= 1024), whichever is larger for the value given.
long long misonet_score_scratch_bytes(int B, int E, int R, long long n_or_F) {
  if (B <= 0 || E <= 0 || R <= 0 || n_or_F <= 0) return -1;
  const long long wave = score_wave_segments(n_or_F) * (2LL * E + 2LL * R + (long long)E * R);
  const long long spec = (n_or_F < 1024 ? n_or_F : 1024) * (long long)E * R;
  return (long long)B * (wave > spec ? wave : spec) * (long long)sizeof(double);
}

static int score_ranges(int B, int E, int R) {
  if (E < 1 || E > 5) return fail(MISONET_EINVAL, "E must be in [1, 5] (got %d): up to 4 speakers and the mixture", E);
  if (R < 1 || R > 4) return fail(MISONET_EINVAL, "R must be in [1, 4] (got %d)", R);
  if (B < 1 || B > 65535) return fail(MISONET_EINVAL, "B must be in [1, 65535] (got %d)", B);
  return MISONET_OK;
}

int misonet_score_wave(const void* est, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                       const float* ref, long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R,
                       long long n, const int* n_valid, double* stats, void* scratch, long long scratch_bytes,
                       misonet_stream stream) {
  if (!est || !ref || !stats || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = score_ranges(B, E, R)) return rc;
  if (n < 1 || n > (1LL << 40)) return fail(MISONET_EINVAL, "n must be in [1, 2^40] (got %lld)", n);
  ScoreViews v;
  if (const int rc = score_views(&v, est, est_is_i16, est_sb, est_ss, est_st, ref, ref_sb, ref_ss, ref_st)) return rc;
  if (const int rc = scratch_fits(scratch_bytes, misonet_score_scratch_bytes(B, E, R, n), "misonet_score_scratch_bytes(B, E, R, n)"))
    return rc;
  HIPCHK(launch_score_wave(v.est, v.ref, B, E, R, n, n_valid, reinterpret_cast<double*>(scratch), stats,
                           reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_score_spec(const void* est, long long est_sb, long long est_ss, long long est_st, const void* ref,
                       long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R, int T, int F,
                       double* pair, int* perm, double* upit, void* scratch, long long scratch_bytes,
                       misonet_stream stream) {
  if (!est || !ref || !pair || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = score_ranges(B, E, R)) return rc;
  if (T < 1) return fail(MISONET_EINVAL, "T must be positive (got %d)", T);
  if (F < 1 || F > 1024) return fail(MISONET_EINVAL, "F must be in [1, 1024] (got %d)", F);
  if ((perm || upit) && E != R)
    return fail(MISONET_EINVAL, "the permutation pick needs as many estimates as references (E %d, R %d)", E, R);
  if (const int rc = view_strides(est_sb, est_ss, est_st, ref_sb, ref_ss, ref_st, "frame")) return rc;
  if (const int rc = scratch_fits(scratch_bytes, misonet_score_scratch_bytes(B, E, R, F), "misonet_score_scratch_bytes(B, E, R, F)"))
    return rc;
  // complex64 views, strides in complex elements, bins contiguous: element (b, f, source, t) at 2 (b sb + source ss + t st + f)
  const float* a = reinterpret_cast<const float*>(est);
  const float* c = reinterpret_cast<const float*>(ref);
  PitArgs p;
  p.a = {a, a + 1, 2 * est_sb, 2, 2 * est_ss, (int)(2 * est_st)};
  p.b = {c, c + 1, 2 * ref_sb, 2, 2 * ref_ss, (int)(2 * ref_st)};
  p.B = B; p.F = F; p.T = T;
  HIPCHK(launch_score_spec(p, E, R, reinterpret_cast<double*>(scratch), pair, perm, upit,
                           reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- BSS-eval energies (bss.hip) -----------------------------------------------------------------------------------------
static int bss_ranges(int B, int E, int R, int Q) {
  if (const int rc = erb_ranges(B, E, R)) return rc;
  if (Q < 16 || Q > 1024 || Q % 16) return fail(MISONET_EINVAL, "Q must be a multiple of 16 in [16, 1024] (got %d)", Q);
  return MISONET_OK;
}

// One size serves both calls: the correlation partials [B][ceil((n + 15) / 4096)][R R + R E + E][Q] and the systems of an item,
// (R Q + 4) R Q + R (Q + 4) Q doubles, whichever is larger.
long long misonet_bss_scratch_bytes(int B, int E, int R, long long n, int Q) {
  if (B < 1 || B > 4096 || E < 1 || E > 4 || R < 1 || R > 4 || Q < 16 || Q > 1024 || Q % 16 || n < 1 || n > (1LL << 24)) return -1;
  const long long corr = bss_corr_segments(n) * ((long long)R * R + (long long)R * E + E) * Q;
  const long long sys = bss_solve_doubles(R, Q);
  return (long long)B * (corr > sys ? corr : sys) * (long long)sizeof(double);
}

int misonet_bss_corr(const void* est, int est_is_i16, long long est_sb, long long est_ss, long long est_st, const float* ref,
                     long long ref_sb, long long ref_ss, long long ref_st, int B, int E, int R, long long n,
                     const int* n_valid, int Q, double* Rrr, double* Rre, double* Eee, void* scratch,
                     long long scratch_bytes, misonet_stream stream) {
  if (!est || !ref || !Rrr || !Rre || !Eee || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = bss_ranges(B, E, R, Q)) return rc;
  if (n < 1 || n > (1LL << 24)) return fail(MISONET_EINVAL, "n must be in [1, 2^24] (got %lld)", n);
  ScoreViews v;
  if (const int rc = score_views(&v, est, est_is_i16, est_sb, est_ss, est_st, ref, ref_sb, ref_ss, ref_st)) return rc;
  if (const int rc = scratch_fits(scratch_bytes, misonet_bss_scratch_bytes(B, E, R, n, Q), "misonet_bss_scratch_bytes(B, E, R, n, Q)"))
    return rc;
  HIPCHK(launch_bss_corr(v.est, v.ref, B, E, R, n, n_valid, Q, reinterpret_cast<double*>(scratch), Rrr, Rre, Eee,
                         reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_bss_solve(const double* Rrr, const double* Rre, const double* Eee, int B, int E, int R, int Q, double* T, double* A,
                      int* info, void* scratch, long long scratch_bytes, misonet_stream stream) {
  if (!Rrr || !Rre || !Eee || !T || !A || !info || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = bss_ranges(B, E, R, Q)) return rc;
  if (const int rc = scratch_fits(scratch_bytes, misonet_bss_scratch_bytes(B, E, R, 1, Q), "misonet_bss_scratch_bytes(B, E, R, 1, Q)"))
    return rc;
  HIPCHK(launch_bss_solve(Rrr, Rre, B, E, R, Q, T, A, info, reinterpret_cast<double*>(scratch),
                          reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- STOI / ESTOI (stoi.hip) ------------------------------------------------------------------------------------------------
static DevTable<double> g_stoi_tab;                   // window, twiddles, polyphase taps
static int get_stoi_table(const double** out) { return score_table(g_stoi_tab, stoi_table_count(), stoi_build_table, out); }

long long misonet_stoi_resampled_len(long long n, int fs) { return stoi_resampled_len(n, fs); }

int misonet_stoi_taps(int fs, double* taps_host) {
  const int nt = stoi_taps(fs);
  if (nt < 0) return fail(MISONET_EINVAL, "fs must be 8000, 10000 or 16000 (got %d)", fs);
  if (taps_host) {
    std::vector<double> t((size_t)stoi_table_count());
    stoi_build_table(t.data());
    const int off = stoi_tap_offset(fs);
    for (int i = 0; i < nt; ++i) taps_host[i] = t[(size_t)off + i];
  }
  return nt;
}

static bool stoi_ranges_ok(int B, int NS, int R, long long n10) {
  return B >= 1 && B <= 4096 && R >= 1 && R <= 4 && NS - R >= 1 && NS - R <= 5 && n10 >= 1 && n10 <= 5 * (1LL << 22);
}

long long misonet_stoi_scratch_bytes(int B, int NS, int R, long long n10) {
  if (!stoi_ranges_ok(B, NS, R, n10)) return -1;
  return (long long)B * stoi_item_doubles(NS, R, n10) * (long long)sizeof(double);
}

int misonet_stoi_resample(const void* est, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                          const float* ref, long long ref_sb, long long ref_ss, long long ref_st, const float* mix,
                          long long mix_sb, long long mix_st, int B, int E, int R, long long n, const int* n_valid, int fs,
                          double* x10, int* len10, misonet_stream stream) {
  if (!est || !ref || !x10 || !len10) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = erb_ranges(B, E, R)) return rc;
  if (fs != 8000 && fs != 10000 && fs != 16000) return fail(MISONET_EINVAL, "fs must be 8000, 10000 or 16000 (got %d)", fs);
  if (n < 1 || n > (1LL << 24)) return fail(MISONET_EINVAL, "n must be in [1, 2^24] (got %lld)", n);
  ScoreViews v;
  if (const int rc = score_views(&v, est, est_is_i16, est_sb, est_ss, est_st, ref, ref_sb, ref_ss, ref_st, mix, mix_sb, mix_st))
    return rc;
  const double* tab;
  if (const int rc = get_stoi_table(&tab)) return rc;
  HIPCHK(launch_stoi_resample(v.est, v.ref, v.mix, B, E, R, n, n_valid, fs, tab, x10, len10,
                              reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

int misonet_stoi_measure(const double* x10, const int* len10, int B, int NS, int R, long long n10, double* out, int* frames,
                         void* scratch, long long scratch_bytes, misonet_stream stream) {
  if (!x10 || !out || !frames || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (!stoi_ranges_ok(B, NS, R, n10))
    return fail(MISONET_EINVAL, "1 <= B <= 4096, 1 <= R <= 4, 1 <= NS - R <= 5, 1 <= n10 <= 5 * 2^22 (got %d, %d, %d, %lld)", B,
                R, NS - R, n10);
  if (const int rc = scratch_fits(scratch_bytes, misonet_stoi_scratch_bytes(B, NS, R, n10), "misonet_stoi_scratch_bytes(B, NS, R, n10)"))
    return rc;
  const double* tab;
  if (const int rc = get_stoi_table(&tab)) return rc;
  HIPCHK(launch_stoi_measure(x10, len10, B, NS, R, n10, tab, out, frames, reinterpret_cast<double*>(scratch),
                             reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- cepstral distance, LLR, fwSegSNR (reverb.hip) -----------------------------------------------------------------------
static DevTable<double> g_reverb_tab;                 // twiddles and, per rate, window, mel triangles, their bin ranges
static int get_reverb_table(const double** out) {
  return score_table(g_reverb_tab, reverb_table_count(), reverb_build_table, out);
}

long long misonet_reverb_frames(long long n, int fs) { return reverb_frames(n, fs); }

long long misonet_reverb_scratch_bytes(int B, int NS, int R, long long n, int fs) {
  if (B < 1 || B > 4096 || R < 1 || R > 4 || NS - R < 1 || NS - R > 5) return -1;
  const long long item = reverb_item_doubles(NS, R, n, fs);
  return item < 0 ? -1 : (long long)B * item * (long long)sizeof(double);
}

int misonet_reverb_measure(const void* est, int est_is_i16, long long est_sb, long long est_ss, long long est_st,
                           const float* ref, long long ref_sb, long long ref_ss, long long ref_st, const float* mix,
                           long long mix_sb, long long mix_st, int B, int E, int R, long long n, const int* n_valid, int fs,
                           double* out, int* count, double* frame, void* scratch, long long scratch_bytes,
                           misonet_stream stream) {
  if (!est || !ref || !out || !count || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (const int rc = erb_ranges(B, E, R)) return rc;
  if (fs != 8000 && fs != 16000) return fail(MISONET_EINVAL, "fs must be 8000 or 16000 (got %d)", fs);
  if (n < 1 || n > (1LL << 24)) return fail(MISONET_EINVAL, "n must be in [1, 2^24] (got %lld)", n);
  ScoreViews v;
  if (const int rc = score_views(&v, est, est_is_i16, est_sb, est_ss, est_st, ref, ref_sb, ref_ss, ref_st, mix, mix_sb, mix_st))
    return rc;
  const int NS = R + E + (mix ? 1 : 0);
  if (const int rc = scratch_fits(scratch_bytes, misonet_reverb_scratch_bytes(B, NS, R, n, fs),
                                  "misonet_reverb_scratch_bytes(B, R + E (+ 1), R, n, fs)"))
    return rc;
  const double* tab;
  if (const int rc = get_reverb_table(&tab)) return rc;
  HIPCHK(launch_reverb_measure(v.est, v.ref, v.mix, B, E, R, n, n_valid, fs, tab, out, count, frame,
                               reinterpret_cast<double*>(scratch), reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

// ---- SRMR (srmr.hip) ---------------------------------------------------------------------------------------------------------
static DevTable<double> g_srmr_tab;   // twiddles and, per rate, window, filter coefficients, transitions, ERB, cutoffs
static int get_srmr_table(const double** out) { return score_table(g_srmr_tab, srmr_table_count(), srmr_build_table, out); }

long long misonet_srmr_frames(long long n, int fs) { return srmr_frames(n, fs); }
int misonet_srmr_chunk(void) { return srmr_chunk(); }

long long misonet_srmr_scratch_bytes(int B, int NS, long long n, int fs) {
  const long long d = srmr_scratch_doubles(B, NS, n, fs);
  return d < 0 ? -1 : d * (long long)sizeof(double);
}

int misonet_srmr_measure(const void* sig, int sig_is_i16, long long sig_sb, long long sig_ss, long long sig_st, const float* mix,
                         long long mix_sb, long long mix_st, int B, int S, long long n, const int* n_valid, int fs, double* out,
                         int* count, double* energy, void* scratch, long long scratch_bytes, misonet_stream stream) {
  if (!sig || !out || !count || !scratch) return fail(MISONET_EINVAL, "null argument");
  if (S < 1 || S > 4) return fail(MISONET_EINVAL, "S must be in [1, 4] (got %d)", S);
  if (B < 1 || B > 4096) return fail(MISONET_EINVAL, "B must be in [1, 4096] (got %d)", B);
  if (fs != 8000 && fs != 16000) return fail(MISONET_EINVAL, "fs must be 8000 or 16000 (got %d)", fs);
  if (n < 1 || n > (1LL << 24)) return fail(MISONET_EINVAL, "n must be in [1, 2^24] (got %lld)", n);
  ScoreViews v;
  if (const int rc = score_views(&v, sig, sig_is_i16, sig_sb, sig_ss, sig_st, nullptr, 0, 0, 1, mix, mix_sb, mix_st)) return rc;
  const int NS = S + (mix ? 1 : 0);
  if (const int rc = scratch_fits(scratch_bytes, misonet_srmr_scratch_bytes(B, NS, n, fs), "misonet_srmr_scratch_bytes(B, S (+ 1), n, fs)"))
    return rc;
  const double* tab;
  if (const int rc = get_srmr_table(&tab)) return rc;
  HIPCHK(launch_srmr_measure(v.est, v.mix, B, S, n, n_valid, fs, tab, out, count, energy,
                             reinterpret_cast<double*>(scratch), reinterpret_cast<hipStream_t>(stream)));
  return MISONET_OK;
}

}  // extern "C"
