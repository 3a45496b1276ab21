"""The glue of the fused pass (csrc/api_pipeline.hip, pipeline_run_impl) on the device's OWN stage outputs, at every geometry the C ABI
admits a sample of: 1-4 speakers, 2-8 microphones, every kind of ref_ch.

Between the networks and the beamformer the pass only selects and moves planes (pack_k / stft_pack_k with the circular shifts,
pit_dist_k / pit_pick_k, compose_sel_k, unpack_k in mode 1, assemble3_k, the est + sel read path of the beamformer, MISO_3 from an
external input in MISO_1's workspace), so against the device's own stages the bound is equality of bits:

    raw        = MISO_1 on the B*M samples rolled by torch.roll on the test's side          (the shift loop of pack_k)
    selection  = read off ex["miso1"] (pipeline_glue_ref.observed_sel) and held to the float64 restatement of the rule
                 (pipeline_glue_ref.expected / check; the clean alignment is forced to a known, per-item different order)
    miso1      = the gather of raw through that selection, in every frame and bin
    bf[:, j]   = Apply_Beamforming(miso1[:, j], mix)
    out        = MISO_3(mix, bf[b, j], miso1[b, j, ref_ch]) over the samples b*S + j
    separate() = miso1, from this Enhancer and from a separation-only one
    enhance_wav(wav) = enhance(stft_hip(wav))
    a workspace of 0xFF bytes and one of zeros give the same bits

No CPU network runs here; the CPU work is the float64 permutation costs.  Two speakers cannot see a wrong selection rule
(tests/test_pipeline_glue.py), hence S >= 3 in most cases; the coverage line of a case says what its selections could tell apart.
Figures: LAB.md, "Fused pass on its own stages"."""
import numpy as np
import pytest
import torch

import pipeline_glue_ref as G
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

F = 129
# (S, M, ref_ch, B, T, forced clean alignment, arithmetic mode or None = the library's default)
# T = 33: one frame in the second 32-frame layout tile; 65: one in the third, Tp = 96; 130: Tp = 160
CASES = [
    (3, 6, 0, 2, 65, True, "f32"),       # the product geometry plus a speaker
    (3, 6, 0, 2, 65, True, "f32w"),
    (3, 6, 0, 2, 65, True, "bf16x6"),
    (3, 6, 5, 2, 65, True, None),        # the last microphone as anchor
    (4, 8, 2, 2, 33, True, None),        # 24 permutations; first layers with 16 and 20 input channels
    (3, 5, 1, 2, 65, False, None),       # odd M; 10 and 14 input channels; clean_sel == nullptr
    (4, 7, 6, 1, 33, False, None),       # 14 and 18 input channels
    (2, 2, 1, 3, 65, True, None),        # the smallest M: a roll of two
    (1, 3, 2, 2, 33, True, None),        # pit_*<1>; two output channels
    (2, 6, 0, 2, 130, True, None),       # the shipped geometry at Tp = 160
]
WEIGHT_SEED = {(3, 6): 2, (4, 8): 6, (3, 5): 8, (2, 2): 7, (4, 7): 5, (1, 3): 3, (2, 6): 0,
               (3, 2): 4}                # S > M: tests/test_gpu_pipeline_steps.py, the refusal of the joint beamformers
WAV_CASES = [CASES[3], CASES[4]]         # the waveform entry: one of them with M = 8
WS_CASE = CASES[4]                       # the workspace's previous contents


def _id(c):
    return f"S{c[0]}-M{c[1]}-ref{c[2]}-B{c[3]}-T{c[4]}-{'clean' if c[5] else 'noclean'}-{c[6] or 'default'}"


_nets = {}


def _networks(S, M, mode):
    """(MISO_1, MISO_3) of a geometry, built once; mode None: the arithmetic a new handle comes with"""
    import misonet_amd as mz
    from misonet_amd import weights as W
    if (S, M) not in _nets:
        seed = WEIGHT_SEED[(S, M)]
        m1 = mz.MISO_1(S, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m1.load_state_dict(W.make_state_dict(W.miso1_spec(num_spks=S, num_ch=M), seed))
        m3 = mz.MISO_3(1, M, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
        m3.load_state_dict(W.make_state_dict(W.miso3_spec(num_ch=M), seed + 100))
        _nets[(S, M)] = (m1.eval(), m3.eval(), m1.precision)
    m1, m3, default = _nets[(S, M)]
    m1.set_precision(mode or default)
    m3.set_precision(mode or default)
    return m1, m3


def mix_of(S, M, B, T):
    """complex64 [B, M, T, 129], item b scaled by 1 + 2 b (per-item indexing of everything the pass keeps per item)"""
    r = np.random.default_rng(9000 + 100 * S + 10 * M + T)
    x = (r.standard_normal((B, M, T, F)) + 1j * r.standard_normal((B, M, T, F))).astype(np.complex64)
    return x * (1.0 + 2.0 * np.arange(B, dtype=np.float32))[:, None, None, None]


def forced_orders(S, B):
    """c[b]: the order the clean references of item b are given in: a transposition for the even items, a 3-cycle (S >= 3) or the
    identity (S = 2) for the odd ones"""
    ident = list(range(S))
    swap = [1, 0] + ident[2:] if S >= 2 else ident
    cyc = [1, 2, 0] + ident[3:] if S >= 3 else ident
    return np.array([swap if b % 2 == 0 else cyc for b in range(B)])


def forced_clean(raw, c, M, ref_ch, seed):
    """clean[b, j] = raw[b*M + ref_ch, c[b, j]] + 0.05 rms noise: sel_clean has to come out as c"""
    B, S = c.shape
    r = np.random.default_rng(seed)
    clean = np.stack([raw[b * M + ref_ch][c[b]] for b in range(B)])
    rms = np.sqrt((np.abs(clean) ** 2).mean(axis=(1, 2, 3), keepdims=True))
    return (clean + 0.05 * rms * (r.standard_normal(clean.shape) + 1j * r.standard_normal(clean.shape))).astype(np.complex64)


def _bits(x):
    return torch.view_as_real(x).contiguous().view(torch.int32) if x.is_complex() else x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _stages(case):
    """everything of a case that its tests share: the networks, the input, the raw MISO_1 outputs, the forced clean references"""
    import misonet_amd as mz
    S, M, ref_ch, B, T, with_clean, mode = case
    m1, m3 = _networks(S, M, mode)
    mix = torch.from_numpy(mix_of(S, M, B, T)).cuda()
    rolled = torch.stack([torch.roll(mix[b], -k, dims=0) for b in range(B) for k in range(M)])     # sample b*M + k
    raw = m1(rolled)
    assert tuple(raw.shape) == (B * M, S, T, F)
    c = forced_orders(S, B)
    clean = torch.from_numpy(forced_clean(raw.cpu().numpy(), c, M, ref_ch, 9500 + T)).cuda() if with_clean else None
    enh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch)
    return m1, m3, enh, mix, raw, clean, c


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_fused_pass_equals_its_own_stages(case):
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import Apply_Beamforming
    S, M, ref_ch, B, T, with_clean, mode = case
    what = _id(case)
    m1, m3, enh, mix, raw, clean, c = _stages(case)
    out, ex = enh.enhance(mix, clean, want_bf=True, want_miso1=True)
    assert tuple(out.shape) == (B, S, T, F) and tuple(ex["bf"].shape) == (B, S, T, F) and tuple(ex["miso1"].shape) == (B, S, M, T, F)
    for k, v in (("out", out), ("bf", ex["bf"]), ("miso1", ex["miso1"])):
        assert bool(torch.isfinite(torch.view_as_real(v)).all()), f"{what}: non-finite {k}"

    # ---- the selection, against the float64 restatement on the device's raw outputs --------------------------------------------
    raw_h, miso1_h = raw.cpu().numpy(), ex["miso1"].cpu().numpy()
    e = G.expected(raw_h, clean.cpu().numpy() if with_clean else None, M, S, ref_ch)
    cov = G.coverage(e["sel_shift"], e["sel_clean"])
    ratio = e["margin_shift"] / np.maximum(2 * e["tol_shift"], 1e-300)
    print(f"[glue-margin] {what}: margin/(2 tol) per (b, m): " + " ".join(f"{v:.3g}" for v in ratio.ravel()))
    obs = G.observed_sel(miso1_h, raw_h, M)
    print(f"[glue-sel] {what}: observed {obs.tolist()} expected {e['sel_final'].tolist()}")
    res = G.check(e, obs, ref_ch, what)
    print(G.coverage_line(what, cov, res))
    if S >= 3:
        # (without clean references sel_clean is the identity: it commutes with everything and is the same for every item)
        assert cov["non_involutive"] > 0, f"{what}: every shift permutation is its own inverse: {e['sel_shift'].tolist()}"
        if with_clean:
            assert cov["non_commuting"] > 0 and cov["clean_differs"], f"{what}: {cov}"
    assert np.array_equal(obs[:, ref_ch], c if with_clean else np.tile(np.arange(S), (B, 1))), (what, obs[:, ref_ch].tolist(), c.tolist())
    if with_clean:
        assert np.array_equal(e["sel_clean"], c), (what, e["sel_clean"].tolist(), c.tolist())

    # ---- the aligned estimates: the gather of raw through the selection, every frame and bin -----------------------------------
    want = torch.from_numpy(G.gather(raw_h, obs, M)).cuda()
    assert _same(ex["miso1"], want), f"{what}: miso1 is not the gather of the raw MISO_1 outputs"

    # ---- the beamformer: the est + sel read path against contiguous tensors ----------------------------------------------------
    mix_bf = mix.permute(0, 3, 1, 2)
    for j in range(S):
        bf_j = Apply_Beamforming(ex["miso1"][:, j].permute(0, 3, 1, 2), mix_bf)
        assert _same(ex["bf"][:, j], bf_j), f"{what}: beamformer output of speaker {j} differs from Apply_Beamforming on miso1[:, {j}]"

    # ---- MISO_3: assembled input (channel order, ref_ch, sel), run from the external input in MISO_1's workspace ---------------
    mix_rep = mix[:, None].expand(B, S, M, T, F).reshape(B * S, M, T, F)                # sample b*S + j
    bf_seg = ex["bf"].reshape(B * S, 1, T, F)
    est_seg = ex["miso1"][:, :, ref_ch].reshape(B * S, 1, T, F)
    for got, ref in zip(G.miso3_inputs(mix.cpu().numpy(), ex["bf"].cpu().numpy(), miso1_h, ref_ch),
                        (mix_rep, bf_seg, est_seg)):
        assert np.array_equal(got, ref.cpu().numpy())                                   # the restatement's order is the one used here
    out3 = m3(mix_rep, bf_seg, est_seg).reshape(B, S, T, F)
    assert _same(out, out3), (f"{what}: the pass's output differs from MISO_3(mix, bf, miso1 at ref_ch) in "
                              f"{int((_bits(out) != _bits(out3)).any(-1).sum())} of {out.numel()} values")

    # ---- the separation path: the same aligned estimates without MISO_3 --------------------------------------------------------
    assert _same(enh.separate(mix, clean), ex["miso1"]), f"{what}: separate() differs from the fused pass's miso1"
    sep = mz.Enhancer(m1, None, num_spks=S, ref_ch=ref_ch)
    assert _same(sep.separate(mix, clean), ex["miso1"]), f"{what}: a separation-only Enhancer differs from the fused pass's miso1"


@pytest.mark.parametrize("case", WAV_CASES, ids=_id)
def test_waveform_entry_equals_spectrogram_entry(case):
    """stft_pack_k with nshift = M (and 1 for the clean references) against stft_hip + pack_k: the same transform kernel"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd.stft import stft_hip
    S, M, ref_ch, B, T, _, mode = case
    m1, m3 = _networks(S, M, mode)
    n = 64 * (T - 1) + 17
    r = np.random.default_rng(9700 + M)
    wav = torch.from_numpy((0.1 * r.standard_normal((B, n, M))).astype(np.float32)).cuda()
    wav[1:] *= 3.0
    clean_wav = torch.from_numpy((0.1 * r.standard_normal((B, n, S))).astype(np.float32)).cuda()
    enh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch)
    out_w, ex_w = enh.enhance_wav(wav, clean_wav, want_bf=True, want_miso1=True)
    mix, clean = stft_hip(wav), stft_hip(clean_wav)
    assert tuple(mix.shape) == (B, M, T, F) and tuple(clean.shape) == (B, S, T, F)
    out_s, ex_s = enh.enhance(mix, clean, want_bf=True, want_miso1=True)
    for k, a, b in (("out", out_w, out_s), ("bf", ex_w["bf"], ex_s["bf"]), ("miso1", ex_w["miso1"], ex_s["miso1"])):
        assert bool(torch.isfinite(torch.view_as_real(a)).all()), (_id(case), k)
        assert _same(a, b), f"{_id(case)}: {k} from the waveform entry differs from the spectrogram entry"
    assert not _same(ex_w["miso1"][:, 0], ex_w["miso1"][:, 1])


def test_pipeline_workspace_previous_contents_do_not_matter():
    """Every index the pass reads (sel_shift, sel_clean, sel_final) and every distance is written earlier in the same pass
    (pipeline_run_impl: pit_dist_k writes all [B*K][F][S][S] partials, pit_pick_k all distances and selections, compose_sel_k all of
    sel_final), so the whole workspace -- not only the networks' part -- may hold anything before a pass."""
    _need_gpu()
    S, M, ref_ch, B, T, _, _ = WS_CASE
    _, _, enh, mix, _, clean, _ = _stages(WS_CASE)
    res = {}
    for byte in (0xFF, 0x00):
        ws = enh.workspace(B, T)
        ws.fill_(byte)
        out, ex = enh.enhance(mix, clean, want_bf=True, want_miso1=True)      # check_nan: the flag word is cleared by the pass itself
        assert enh.workspace(B, T).data_ptr() == ws.data_ptr()
        res[byte] = {"out": out.clone(), "bf": ex["bf"].clone(), "miso1": ex["miso1"].clone()}
    for k in res[0]:
        assert bool(torch.isfinite(torch.view_as_real(res[0xFF][k])).all()), f"{k}: non-finite after a workspace of 0xFF bytes"
        assert _same(res[0xFF][k], res[0][k]), f"{k}: a workspace of 0xFF bytes and one of zeros give different bits"
