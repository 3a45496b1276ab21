"""Full-size GPU parity (BASELINE.json configs[1]-[3]: T = 1001 frames = 4 s at 16 kHz, batch 16 -- the reference's unit
of work is the full chunk, tester.py:917-939, config/NN_BSS.yml:72-78): the bench batch itself runs through
``Enhancer.enhance`` in every arithmetic mode and utterances picked from inside the batch are compared stage by stage
(MISO1 at all mics, both beamformer outputs, MISO3) with the CPU oracle run utterance by utterance; Apply_Beamforming
alone at [1,129,6,1001].  Also the ill-conditioned-statistics case for the modes that fold the instance norm into the
weights."""
import numpy as np
import pytest
import torch

from conftest import golden, rel_l2, mag_parity, modes
from test_gpu_parity import _assert_parity, _utt_inputs, _need_gpu

pytestmark = pytest.mark.gpu

B_BENCH, T_FULL = 16, 1001
CHECK_UTTS = (3, 12)               # positions inside the batch of 16 (different XCD / tile-walk positions)
# measured per-mode bound on the end-to-end magnitude rel-L2 (tolerance of the path: 1e-3); fp32-faithful modes must be
# indistinguishable from each other
MODE_TOL = {"f32": 4e-5, "f32w": 4e-5, "bf16x6": 4e-5}   # measured: <= 1.9e-5


def _modes():
    return modes("f32", "f32w", "bf16x6")


@pytest.fixture(scope="module")
def bench_batch(sd1, sd3):
    """the 16 synthetic utterances of bench.py (rank 0) + the oracle's result for CHECK_UTTS (about 10 s each)"""
    _need_gpu()
    from oracle import pipeline_oracle
    ins = [_utt_inputs(u, T_FULL) for u in range(B_BENCH)]
    refs = {u: pipeline_oracle.enhance_utterance(ins[u][0], ins[u][1], sd1, sd3, ref_ch=0) for u in CHECK_UTTS}
    mix = torch.from_numpy(np.stack([i[0] for i in ins]))
    clean = torch.from_numpy(np.stack([i[1] for i in ins]))
    return mix, clean, refs


@pytest.mark.parametrize("mode", modes("f32", "f32w", "bf16x6"))
def test_full_size_batch16_pipeline_vs_oracle(bench_batch, sd1, sd3, mode):
    import misonet_amd as mz
    from misonet_amd import weights as W
    if mode not in _modes():
        pytest.skip(f"mode {mode} not built")
    mix, clean, refs = bench_batch
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    m1.eval().set_precision(mode)
    m3.eval().set_precision(mode)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out, extra = enh.enhance(mix.cuda(), clean.cuda(), want_bf=True, want_miso1=True)
    assert tuple(out.shape) == (B_BENCH, 2, T_FULL, 129)
    tol = MODE_TOL[mode]
    for u in CHECK_UTTS:
        r = refs[u]
        _assert_parity(extra["miso1"][u].cpu().numpy(), r["miso1"], f"[{mode}] utt {u} miso1 (all mics) T=1001 B=16")
        _assert_parity(extra["bf"][u].cpu().numpy(), r["bf"], f"[{mode}] utt {u} bf T=1001 B=16")
        _assert_parity(out[u].cpu().numpy(), r["out"], f"[{mode}] utt {u} miso3 T=1001 B=16")
        e = mag_parity(out[u].cpu().numpy(), r["out"])[0]
        assert e <= tol, f"[{mode}] utt {u}: end-to-end rel-L2 {e:.3e} above the mode's measured bound {tol:.0e}"
    # utterance 0 of the batch against the REAL reference at full size (G12, oracle/gen_golden_full.py)
    _check_g12(extra["miso1"][0].cpu().numpy()[:, 0], extra["bf"][0].cpu().numpy(), out[0].cpu().numpy(),
               f"[{mode}] utt 0 of the batch of 16", ms_tol=max(1e-4, 3 * tol))
    del enh, m1, m3
    torch.cuda.empty_cache()


def _check_g12(miso1_ref, bf, out, what, ms_tol=1e-4):
    """stage outputs [2, T, F] of bench utterance 0 against the reference's own run (every 16th frame + all magnitude sums)"""
    g = golden("g12_fullsize_T1001.npz")
    st = int(g["frame_step"])
    assert int(g["frames"]) == T_FULL and int(g["utt"]) == 0
    for name, got in (("miso1_ref", miso1_ref), ("bf", bf), ("out", out)):
        _assert_parity(got[:, ::st], g[name + "_frames"], f"{what}: {name} vs reference golden G12")
        ms = np.abs(got).astype(np.float64).sum(-1)
        e = rel_l2(ms, g[name + "_magsum"])
        print(f"[parity] {what}: {name} per-frame magnitude sums of all {T_FULL} frames vs G12: {e:.3e}")
        assert e <= ms_tol, f"{what}: {name} per-frame magnitude sums differ by {e:.3e}"


@pytest.mark.parametrize("mode", ["f32", "f32w", "bf16x6"])
def test_full_size_single_utterance_vs_reference_golden(sd1, sd3, mode):
    """B = 1 (the reference harness' own batch size, config/NN_BSS.yml:108-111) at T = 1001 against G12: MISO_1.forward
    (model.py:76-111) and the whole body of Tester_Enhance.inference (tester.py:846-975) incl. the int16 waves, all from
    the real reference run on the bench's utterance 0 in the build container."""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    g = golden("g12_fullsize_T1001.npz")
    st = int(g["frame_step"])
    mx, cl = _utt_inputs(0, T_FULL)
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    m1.eval().set_precision(mode)
    m3.eval().set_precision(mode)
    y = m1(torch.from_numpy(mx[None]).cuda()).cpu().numpy()[0]
    _assert_parity(y[:, ::st], g["miso1_fwd_frames"], f"[{mode}] MISO_1.forward T=1001 vs reference golden G12")
    assert rel_l2(np.abs(y).astype(np.float64).sum(-1), g["miso1_fwd_magsum"]) <= 1e-4
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out, extra = enh.enhance(torch.from_numpy(mx[None]).cuda(), torch.from_numpy(cl[None]).cuda(), want_bf=True, want_miso1=True)
    _check_g12(extra["miso1"][0].cpu().numpy()[:, 0], extra["bf"][0].cpu().numpy(), out[0].cpu().numpy(), f"[{mode}] B = 1")
    wav = enh.to_wav_int16([out[0]], gap=0)                              # [2, 64000] int16
    assert wav.shape == (2, (T_FULL - 1) * 64)
    for s in range(2):
        d = np.abs(wav[s][::16].astype(np.int32) - g["wav_dec16"][s].astype(np.int32))
        print(f"[wav] [{mode}] spk{s} vs the reference's int16 wave (every 16th sample): max |diff| = {d.max()} LSB")
        assert d.max() <= 1
        a = np.abs(wav[s].astype(np.int64)).reshape(-1, 1000).sum(-1)
        assert np.max(np.abs(a - g["wav_abssum_1000"][s])) <= 1000        # all samples: <= 1 LSB each
    del enh, m1, m3
    torch.cuda.empty_cache()


def test_full_size_mvdr_alone():
    """Apply_Beamforming at the reference's call shape [1,129,6,1001] (tester.py:920-924)."""
    _need_gpu()
    from misonet_amd import Apply_Beamforming
    from oracle import mvdr_oracle
    mx, cl = _utt_inputs(5, T_FULL)
    mix = np.transpose(mx, (2, 0, 1))[None]                              # [1,F,M,T]
    r = np.random.default_rng(55)
    # a plausible source estimate: the clean image of speaker 0 at every mic, perturbed
    src = (0.6 * mix + 0.05 * (r.standard_normal(mix.shape) + 1j * r.standard_normal(mix.shape))).astype(np.complex64)
    out, dbg = Apply_Beamforming(src, mix, return_debug=True)
    ref = mvdr_oracle.mvdr_parts(src, mix, dtype=np.complex128)
    e_s = rel_l2(dbg["steer1"].cpu().numpy(), ref["steer1"])
    e_w = rel_l2(dbg["w"].cpu().numpy(), ref["w"])
    e_o = rel_l2(out.numpy(), ref["out"])
    print(f"[mvdr full size] steer {e_s:.3e} w {e_w:.3e} out {e_o:.3e}")
    assert tuple(out.shape) == (1, T_FULL, 129)
    assert e_s < 1e-4 and e_w < 1e-4 and e_o < 1e-4


@pytest.mark.parametrize("dc,bias_sigma", [(5.0, 2.0), (25.0, 4.0)])
def test_folded_norm_ill_conditioned_statistics(sd1, dc, bias_sigma):
    """The DMA dataflows fold the instance norm of a layer's input into the weights (W' = W * rstd, shift table): the
    products W' * x cancel against the shift when |mean| >> std.  Inputs with a DC offset per channel and weights with
    large biases (post-ELU means far from zero) make the whole forward ill-conditioned for ANY float32 implementation,
    so the ground truth here is the oracle run in float64 and the yardstick is the exact-f32 mode's distance from it.
    bf16x6 (exact operands, fp32-faithful) must stay at that yardstick."""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    from oracle import miso_oracle
    sd = {k: v.copy() for k, v in sd1.items()}
    r = np.random.default_rng(17)
    for k in sd:
        if k.endswith(".bias") and sd[k].ndim == 1:
            sd[k] = (sd[k] + bias_sigma * r.standard_normal(sd[k].shape)).astype(np.float32)
    T = 96
    x = (r.standard_normal((2, 6, T, 129)) + 1j * r.standard_normal((2, 6, T, 129))).astype(np.complex64)
    x += np.complex64(dc + 0.4j * dc)
    with miso_oracle.precision(torch.float64):
        truth = np.concatenate([miso_oracle.miso1_forward(torch.from_numpy(x[b:b + 1]).to(torch.complex128), sd).numpy()
                                for b in range(2)])
    o32 = np.concatenate([miso_oracle.miso1_forward(torch.from_numpy(x[b:b + 1]), sd).numpy() for b in range(2)])
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd)
    m1.eval()
    err = {"oracle_f32": mag_parity(o32, truth)[0]}
    for mode in _modes():
        m1.set_precision(mode)
        err[mode] = mag_parity(m1(torch.from_numpy(x).cuda()).cpu().numpy(), truth)[0]
    print(f"[ill-conditioned dc={dc} bias_sigma={bias_sigma}] error vs float64 truth: " +
          "  ".join(f"{k} {v:.3e}" for k, v in err.items()))
    # yardstick: the exact-f32 MFMA mode of this library under the same conditioning (the float32 oracle is reported too)
    assert all(np.isfinite(v) for v in err.values()), err
    assert err["bf16x6"] <= 4.0 * err["f32"] + 2e-6, err
    # Winograd's transforms add rounding steps with cancellation: under bad conditioning it may sit above the direct form, not
    # beyond the float32 class
    assert np.isfinite(err["f32w"]) and err["f32w"] <= 6.0 * err["f32"] + 4e-6, err


@pytest.mark.parametrize("mode", ["bf16x6", "f32w"])
def test_large_batch_offsets_beyond_4_gib(sd1, sd3, mode):
    """40 utterances at T = 1001 (a 64 GB workspace: sample blocks far beyond 32-bit byte offsets) -- two distinct utterances
    repeated: every copy returns the bits of the first one (exact statistics, per-sample blocks), wherever it sits.  In the
    library default and in "f32w" (the persistent Winograd kernel walks 240 / 80 samples with its own descriptors)."""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    if torch.cuda.get_device_properties(0).total_memory < 120e9:
        pytest.skip("needs > 120 GB of device memory")
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    enh = mz.Enhancer(m1.eval().set_precision(mode), m3.eval().set_precision(mode), num_spks=2, ref_ch=0)
    a, b = _utt_inputs(1, 1001), _utt_inputs(2, 1001)
    mix = torch.from_numpy(np.stack([a[0], b[0]])).cuda().repeat(20, 1, 1, 1)
    clean = torch.from_numpy(np.stack([a[1], b[1]])).cuda().repeat(20, 1, 1, 1)
    out = enh.enhance(mix, clean)
    ref = enh.enhance(mix[:2].contiguous(), clean[:2].contiguous())
    for i in (2, 17, 38, 39):
        assert torch.equal(out[i], ref[i % 2]), i
    del out, mix, clean
    enh._ws.clear()
    torch.cuda.empty_cache()
