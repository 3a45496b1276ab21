// C ABI of the fused pipeline (include/misonet.h, misonet_pipeline_*): MISO1 over the circular shifts -> alignments -> beamformer
// -> MISO3 in one workspace, from spectra or straight from the waveform.  Host code only.
#include "net.hpp"

#include <algorithm>

using namespace mn;

struct misonet_pipeline {
  misonet_net* n1;
  misonet_net* n3;
  int M, S, ref_ch;
  float epsi;
  misonet_bf_opts bf;      // the beamformer of step 5 (misonet_pipeline_set_beamformer); create: the defaults with epsi
  bool use_wpd;            // step 5 is WPD (misonet_pipeline_set_wpd) with the options below, bf is kept for the way back
  misonet_wpd_opts wpd;
  bool use_refine;         // step 4b: guided spatial clustering between the alignments and step 5 (misonet_pipeline_set_refine)
  misonet_cacgmm_opts refine;
  bool use_joint;          // step 5 is one joint beamformer for all speakers (misonet_pipeline_set_joint); bf / wpd are kept
  misonet_jbf_opts joint;
};

struct PipeLayout {
  Layout L1, L3;
  long long off_ws1, off_ws3, off_clean, off_dist, off_sel, off_mvdr, total;
  long long clean_bstride;
  // step 4b, only with refine set: the initial and the refined masks [B][S + 1][F][T], the refined images in the planar estimate
  // layout [B M][2 S][F][Tp], the workspace of launch_cacgmm
  long long off_rmask0, off_rmask, off_rimg, off_rws, rimg_bstride;
};

static PipeLayout pipe_layout(const misonet_pipeline* p, int B, int T) {
  PipeLayout P;
  // MISO3 runs in MISO1's workspace (MISO1 is finished when MISO3 starts; what the steps in between read of it -- its input
  // and output planes -- is consumed before the MISO3 forward writes anything): only the MISO3 INPUT, which those steps
  // build while MISO1's planes are still being read, has its own memory
  P.L1 = make_layout(p->n1, B * p->M, T);
  if (p->n3) P.L3 = make_layout(p->n3, B * p->S, T, true);
  else { P.L3 = Layout(); P.L3.total_bytes = 0; }       // separation-only pipeline: no MISO3 workspace, no MISO3 input
  const int F = p->n1->cfg.n_freq, Tp = P.L1.Tp;
  long long o = 256;                                   // [0]: nan flag
  // PIT distances [B*M + B][S][S] followed by their per-bin partials [B*M + B][F][S][S] (mvdr.hip pit_dist_k)
  P.off_dist = o;  o += align_up((long long)(B * p->M + B) * p->S * p->S * (F + 1) * 8, 256);
  P.off_sel = o;   o += align_up((long long)(B * p->M * p->S * 2 + B * p->S) * 4, 256);
  P.off_mvdr = o;  o += align_up(p->use_joint ? jbf_ws_bytes(B, p->S, F, p->M, p->joint.kind)
                                 : p->use_wpd ? wpd_ws_bytes(B, p->S, F, p->M, p->wpd.taps)
                                              : bf_ws_bytes(B, p->S, F, p->M, p->bf.kind), 256);
  P.clean_bstride = (long long)2 * p->S * F * Tp;
  P.off_clean = o; o += align_up(P.clean_bstride * B * 4, 256);
  P.L3.in_ext_bstride = p->n3 ? (long long)p->n3->cfg.in_ch * F * Tp : 0;
  const long long in3_bytes = align_up(P.L3.in_ext_bstride * B * p->S * 4, 256);
  P.off_ws1 = o;   o += align_up(std::max(P.L1.total_bytes, P.L3.total_bytes), 256);
  P.off_ws3 = P.off_ws1;
  P.L3.in_ext_off = o - P.off_ws3;                     // relative to the (shared) workspace base
  o += in3_bytes;
  P.off_rmask0 = P.off_rmask = P.off_rimg = P.off_rws = 0;
  P.rimg_bstride = (long long)2 * p->S * F * Tp;
  if (p->use_refine) {                                 // behind everything else: nothing before it moves
    const long long mask_bytes = align_up((long long)B * (p->S + 1) * F * T * 4, 256);
    P.off_rmask0 = o; o += mask_bytes;
    P.off_rmask = o;  o += mask_bytes;
    P.off_rimg = o;   o += align_up(P.rimg_bstride * B * p->M * 4, 256);
    P.off_rws = o;    o += align_up(cacgmm_ws_bytes(B, p->S + 1, F, p->M), 256);
  }
  P.total = o;
  return P;
}

extern "C" {

int misonet_pipeline_create(misonet_net* n1, misonet_net* n3, int num_mic, int num_spk, int ref_ch, float epsi,
                            misonet_pipeline** out) {
  // n3 == NULL: a separation-only pipeline (MISO1_Inference + alignments: the body shared by the reference's
  // Tester_Beamforming, tester.py:340-449) -- misonet_pipeline_run then only accepts out == NULL, bf_out == NULL
  if (!n1 || !out) return fail(MISONET_EINVAL, "null argument");
  if (num_spk < 1 || num_spk > 4) return fail(MISONET_EINVAL, "num_spk must be in [1, 4] (PIT enumerates num_spk! permutations)");
  if (num_mic < 2 || num_mic > 8) return fail(MISONET_EINVAL, "num_mic must be in [2, 8]");
  if (ref_ch < 0 || ref_ch >= num_mic) return fail(MISONET_EINVAL, "ref_ch out of range");
  if (n1->cfg.in_ch != 2 * num_mic || n1->cfg.out_ch != 2 * num_spk)
    return fail(MISONET_EINVAL, "MISO_1 geometry does not match num_mic/num_spk");
  if (n3 && (n3->cfg.in_ch != 2 * (num_mic + 2) || n3->cfg.out_ch != 2))
    return fail(MISONET_EINVAL, "MISO_3 geometry must be in_ch = 2*(num_mic+2), out_ch = 2");
  { int rf = misonet_frontend_init(); if (rf) return rf; }     // STFT / iSTFT tables: never allocated inside an asynchronous call
  misonet_pipeline* p = new misonet_pipeline{n1, n3, num_mic, num_spk, ref_ch, epsi};
  misonet_bf_opts_default(&p->bf);
  p->bf.epsi = epsi;
  *out = p;
  return MISONET_OK;
}

int misonet_pipeline_set_beamformer(misonet_pipeline* p, const misonet_bf_opts* opts) {
  if (!p) return fail(MISONET_EINVAL, "null argument");
  { int r = bf_opts_check(opts, p->M); if (r) return r; }
  p->bf = *opts;
  return MISONET_OK;
}
int misonet_pipeline_set_wpd(misonet_pipeline* p, const misonet_wpd_opts* opts) {
  if (!p) return fail(MISONET_EINVAL, "null argument");
  if (!opts) { p->use_wpd = false; return MISONET_OK; }
  { int r = wpd_opts_check(opts, p->M, -1); if (r) return r; }
  p->wpd = *opts;
  p->use_wpd = true;
  return MISONET_OK;
}
int misonet_pipeline_set_refine(misonet_pipeline* p, const misonet_cacgmm_opts* opts) {
  if (!p) return fail(MISONET_EINVAL, "null argument");
  if (!opts) { p->use_refine = false; return MISONET_OK; }
  { int r = cacgmm_opts_check(opts); if (r) return r; }
  p->refine = *opts;
  p->use_refine = true;
  return MISONET_OK;
}
int misonet_pipeline_set_joint(misonet_pipeline* p, const misonet_jbf_opts* opts) {
  if (!p) return fail(MISONET_EINVAL, "null argument");
  if (!opts) { p->use_joint = false; return MISONET_OK; }
  { int r = jbf_opts_check(opts, p->M, p->S); if (r) return r; }
  p->joint = *opts;
  p->use_joint = true;
  return MISONET_OK;
}
int misonet_pipeline_destroy(misonet_pipeline* p) { delete p; return MISONET_OK; }

long long misonet_pipeline_workspace_bytes(const misonet_pipeline* p, int B, int T) {
  if (!p || B <= 0 || T <= 0) return -1;
  return pipe_layout(p, B, T).total;
}

static int pipeline_run_impl(misonet_pipeline* p, const void* mix, const void* clean, const float* wav,
                             const float* clean_wav, int n_samples, int B, int T, void* out, void* bf_out,
                             void* miso1_out, void* ws, long long ws_bytes, misonet_stream stream) {
  if (!p || (!mix && !wav) || (!out && !miso1_out) || !ws) return fail(MISONET_EINVAL, "null argument");
  if (!p->n1->committed || (p->n3 && !p->n3->committed)) return fail(MISONET_ESTATE, "networks not committed");
  if (!p->n3 && (out || bf_out))
    return fail(MISONET_ESTATE, "this pipeline was created without MISO_3 (separation only): out and bf_out must be NULL");
  if (B <= 0 || T <= 0) return fail(MISONET_EINVAL, "B and T must be positive");
  if (p->use_wpd && !p->use_joint && out) {
    int rw = wpd_opts_check(&p->wpd, p->M, T);
    if (!rw) rw = wpd_ready();
    if (rw) return rw;
  }
  const PipeLayout P = pipe_layout(p, B, T);
  if (ws_bytes < P.total) return fail(MISONET_ENOMEM, "workspace %lld < %lld bytes", ws_bytes, P.total);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>(ws);
  void* ws1 = base + P.off_ws1;
  void* ws3 = base + P.off_ws3;
  const int M = p->M, S = p->S, F = p->n1->cfg.n_freq, Tp = P.L1.Tp;
  misonet_net *n1 = p->n1, *n3 = p->n3;
  double* dist_shift = reinterpret_cast<double*>(base + P.off_dist);          // [B*M][S][S]
  double* dist_clean = dist_shift + (long long)B * M * S * S;                  // [B][S][S]
  double* part_shift = dist_clean + (long long)B * S * S;                      // [B*M][F][S][S]
  double* part_clean = part_shift + (long long)B * M * F * S * S;              // [B][F][S][S]
  int* sel_shift = reinterpret_cast<int*>(base + P.off_sel);                   // [B*M][S]
  int* sel_final = sel_shift + (long long)B * M * S;                           // [B*M][S]
  int* sel_clean = sel_final + (long long)B * M * S;                           // [B][S]
  HIPCHK(hipMemsetAsync(base, 0, 256, s));                                     // nan flag

  // 1. MISO1_Inference: the M circular shifts as one batch of B*M samples (tester.py:1033-1051)
  float* in1 = buf_ptr(P.L1, ws1, B_IN);
  const long long in1_bs = bstride(n1, P.L1, B_IN);
  const float* tw = nullptr;
  if (wav) { int rt = get_twiddles(&tw); if (rt) return rt; }
  if (wav) HIPCHK(launch_stft_pack(wav, B, n_samples, M, T, tw, in1, in1_bs, Tp, F, 0, M, M, s));
  else HIPCHK(launch_pack(reinterpret_cast<const float2*>(mix), B, M, T, F, in1, in1_bs, Tp, 0, M, M, s));
  int r = forward_planar(n1, P.L1, ws1, s);
  if (r) return r;
  float* out1 = buf_ptr(P.L1, ws1, B_OUT);
  const long long out1_bs = bstride(n1, P.L1, B_OUT);
  const long long plane = (long long)F * Tp;

  // 2. align the speakers of every shift to the reference-mic forward (tester.py:1043-1065)
  {
    PitArgs q;
    const float* anc = out1 + (long long)p->ref_ch * out1_bs;
    q.a = {anc, anc + S * plane, (long long)M * out1_bs, Tp, plane, 1};
    q.b = {out1, out1 + S * plane, out1_bs, Tp, plane, 1};
    q.B = B; q.F = F; q.T = T;
    HIPCHK(launch_pit_dist_k(q, S, M, part_shift, s));
    HIPCHK(launch_pit_pick(part_shift, F, S, B * M, dist_shift, sel_shift, s));
  }
  // 3. align to the clean references at ref_ch (tester.py:889-915), optional
  if (clean || clean_wav) {
    float* cl = reinterpret_cast<float*>(base + P.off_clean);
    if (clean_wav) HIPCHK(launch_stft_pack(clean_wav, B, n_samples, S, T, tw, cl, P.clean_bstride, Tp, F, 0, S, 1, s));
    else HIPCHK(launch_pack(reinterpret_cast<const float2*>(clean), B, S, T, F, cl, P.clean_bstride, Tp, 0, S, 1, s));
    // anchors = clean sources; candidates = shift-aligned ref-mic estimates.  The ref-mic forward is never
    // permuted by step 2 (its distance matrix has a zero diagonal), so the raw OUT1 planes are the candidates.
    PitArgs q;
    const float* cand = out1 + (long long)p->ref_ch * out1_bs;
    q.a = {cl, cl + S * plane, P.clean_bstride, Tp, plane, 1};
    q.b = {cand, cand + S * plane, (long long)M * out1_bs, Tp, plane, 1};
    q.B = B; q.F = F; q.T = T;
    HIPCHK(launch_pit_dist_k(q, S, 1, part_clean, s));
    HIPCHK(launch_pit_pick(part_clean, F, S, B, dist_clean, sel_clean, s));
  }
  HIPCHK(launch_compose_sel(sel_shift, (clean || clean_wav) ? sel_clean : nullptr, B, M, S, sel_final, s));

  if (out) {   // out == NULL: separation only (MISO1_Inference + alignments), e.g. for the utterance-wise beamformer
    // 4. MISO3 input = [mixture | beamformer | MISO1 estimate at ref_ch] (tester.py:936-939), B*S samples
    float* in3 = buf_ptr(P.L3, ws3, B_IN);
    const long long in3_bs = bstride(n3, P.L3, B_IN);
    HIPCHK(launch_assemble3(in1, in1_bs, out1, out1_bs, sel_final, B, M, S, p->ref_ch, F, Tp, in3, in3_bs, s));

    // 4b. guided spatial clustering (optional): initial masks from the aligned MISO1 planes and the shift-0 mixture, the cACGMM,
    // and its images gamma_s Y as the source estimate of step 5.  MISO3's third input (above) and miso1_out stay the raw estimate
    const float* est5 = out1;
    long long est5_bs = out1_bs;
    const int* sel5 = sel_final;
    if (p->use_refine) {
      float* m0 = reinterpret_cast<float*>(base + P.off_rmask0);
      float* rimg = reinterpret_cast<float*>(base + P.off_rimg);
      MaskArgs ma;
      ma.mix = {in1, in1 + (long long)M * plane, (long long)M * in1_bs, Tp, plane, 1};
      ma.est = out1; ma.est_bstride = out1_bs; ma.sel = sel_final;
      ma.src = {nullptr, nullptr, 0, 0, 0, 1}; ma.src_ss = 0;
      ma.S = S; ma.B = B; ma.F = F; ma.M = M; ma.T = T; ma.Tp = Tp;
      ma.masks = m0;
      HIPCHK(launch_masks_from_est(ma, s));
      CacgmmArgs ca;
      ca.mix = ma.mix;
      ca.init = m0; ca.masks = reinterpret_cast<float*>(base + P.off_rmask);
      ca.img = {rimg, rimg + (long long)S * plane, (long long)M * P.rimg_bstride, plane, Tp, P.rimg_bstride, 1, Tp};
      ca.B = B; ca.K = S + 1; ca.F = F; ca.M = M; ca.T = T;
      ca.iters = p->refine.iterations; ca.guided = p->refine.prior; ca.diag_load = p->refine.diag_load;
      ca.prior_floor = p->refine.prior_floor;
      HIPCHK(launch_cacgmm(ca, base + P.off_rws, s));
      est5 = rimg; est5_bs = P.rimg_bstride; sel5 = nullptr;
    }

    // 5. MVDR per aligned speaker (tester.py:917-924, 1071-1136); writes the beamformer planes of the MISO3 input
    if (p->use_joint) {   // ... or one joint beamformer for all speakers, on the same views and the same planes
      JbfArgs a;
      a.mix = {in1, in1 + (long long)M * plane, (long long)M * in1_bs, Tp, plane, 1};
      a.est = est5; a.est_bstride = est5_bs; a.sel = sel5;
      a.src = {nullptr, nullptr, 0, 0, 0, 1}; a.src_ss = 0;
      a.S = S; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = Tp;
      jbf_opts_apply(p->joint, a);
      COut co = {in3 + (long long)M * plane, in3 + (long long)(2 * M + 2) * plane, (long long)S * in3_bs, in3_bs, 1, Tp};
      ProfScope ps(s, PK_MVDR);
      HIPCHK(launch_jbf(a, co, base + P.off_mvdr, s));
    } else if (p->use_wpd) {   // ... or WPD on the same views and the same planes
      WpdArgs a;
      a.mix = {in1, in1 + (long long)M * plane, (long long)M * in1_bs, Tp, plane, 1};
      a.est = est5; a.est_bstride = est5_bs; a.sel = sel5;
      a.src = {nullptr, nullptr, 0, 0, 0, 1};
      a.S = S; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = Tp;
      wpd_opts_apply(p->wpd, a);
      COut co = {in3 + (long long)M * plane, in3 + (long long)(2 * M + 2) * plane, (long long)S * in3_bs, in3_bs, 1, Tp};
      ProfScope ps(s, PK_MVDR);
      HIPCHK(launch_wpd(a, co, base + P.off_mvdr, s));
    } else {
      MvdrArgs a;
      a.mix = {in1, in1 + (long long)M * plane, (long long)M * in1_bs, Tp, plane, 1};   // shift-0 sample = un-rolled mixture
      a.est = est5; a.est_bstride = est5_bs; a.sel = sel5;
      a.src = {nullptr, nullptr, 0, 0, 0, 1};
      a.S = S; a.B = B; a.F = F; a.M = M; a.T = T; a.Tp = Tp;
      bf_opts_apply(p->bf, a);
      COut co = {in3 + (long long)M * plane, in3 + (long long)(2 * M + 2) * plane, (long long)S * in3_bs, in3_bs, 1, Tp};
      ProfScope ps(s, PK_MVDR);
      HIPCHK(launch_mvdr(a, co, base + P.off_mvdr, s));
    }
    // (the aligned MISO1 estimates leave the shared workspace before MISO3 overwrites it)
    if (miso1_out)
      HIPCHK(launch_unpack_ex(out1, out1_bs, Tp, S, T, F, 0, S, 1, M, sel_final, reinterpret_cast<float2*>(miso1_out),
                              B * S * M, reinterpret_cast<int*>(base), s));
    // 6. MISO3 per speaker (tester.py:1231-1244), in MISO1's workspace
    r = forward_planar(n3, P.L3, ws3, s);
    if (r) return r;
    HIPCHK(launch_unpack(buf_ptr(P.L3, ws3, B_OUT), bstride(n3, P.L3, B_OUT), Tp, 1, T, F, reinterpret_cast<float2*>(out),
                         B * S, reinterpret_cast<int*>(base), s));
    if (bf_out)
      HIPCHK(launch_unpack_ex(in3, in3_bs, Tp, 1, T, F, M, 2 * M + 2, 0, 1, nullptr,
                              reinterpret_cast<float2*>(bf_out), B * S, reinterpret_cast<int*>(base), s));
  } else if (miso1_out) {
    HIPCHK(launch_unpack_ex(out1, out1_bs, Tp, S, T, F, 0, S, 1, M, sel_final, reinterpret_cast<float2*>(miso1_out),
                            B * S * M, reinterpret_cast<int*>(base), s));
  }
  return MISONET_OK;
}

int misonet_pipeline_run(misonet_pipeline* p, const void* mix, const void* clean, int B, int T, void* out, void* bf_out,
                         void* miso1_out, void* ws, long long ws_bytes, misonet_stream stream) {
  return pipeline_run_impl(p, mix, clean, nullptr, nullptr, 0, B, T, out, bf_out, miso1_out, ws, ws_bytes, stream);
}

int misonet_pipeline_run_wav(misonet_pipeline* p, const float* wav, const float* clean_wav, int B, int n_samples,
                             void* out, void* bf_out, void* miso1_out, void* ws, long long ws_bytes,
                             misonet_stream stream) {
  if (n_samples <= 0) return fail(MISONET_EINVAL, "n_samples must be positive");
  return pipeline_run_impl(p, nullptr, nullptr, wav, clean_wav, n_samples, B, misonet_stft_frames(n_samples), out, bf_out,
                           miso1_out, ws, ws_bytes, stream);
}

int misonet_pipeline_check(misonet_pipeline* p, const void* ws, misonet_stream stream) {
  if (!p || !ws) return fail(MISONET_EINVAL, "null argument");
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, ws, sizeof(int), hipMemcpyDeviceToHost, reinterpret_cast<hipStream_t>(stream)));
  HIPCHK(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  if (flag) return fail(MISONET_ENAN, "NaN in pipeline output");
  return MISONET_OK;
}

}  // extern "C"
