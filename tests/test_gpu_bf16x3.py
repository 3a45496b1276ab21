"""GPU parity of the split-bf16 precision mode "bf16x6" (fp32-faithful: exact 3-way split, six terms, conv_bf16x6.hip) against
the same goldens / oracle and the same 1e-3 tolerance as the exact-f32 mode.  (Test and file names say bf16x3 for history: the
two-piece modes these tests were first written for were measured and dropped, LAB.md.)  tests/test_gpu_bf16x6.py holds bf16x6 to the f32 mode's own error level on top of this."""
import numpy as np
import pytest
import torch

from conftest import golden, rel_l2, mag_parity, modes
from test_gpu_parity import _assert_parity, _utt_inputs, _need_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=modes("bf16x6"))
def nets_bf(request, sd1, sd3):
    _need_gpu()
    PREC = request.param
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m1.eval().set_precision(PREC)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    m3.eval().set_precision(PREC)
    return m1, m3


def test_bf16x3_stage_taps(nets_bf, sd1, request):
    from oracle import miso_oracle
    m1, _ = nets_bf
    g = golden("g1_miso1_T32.npz")
    x = torch.from_numpy(g["x"])
    taps = {}
    y_ref = miso_oracle.miso1_forward(x, sd1, taps).numpy()
    m1.keep_activations(True)                          # taps need un-shared activation buffers
    request.addfinalizer(lambda: m1.keep_activations(False))
    y = m1(x.cuda()).cpu().numpy()
    for nm in ["enc0_conv"] + [f"enc{b}" for b in range(7)] + ["tcn_out"] + [f"dec{b}" for b in range(7)]:
        ref = taps[nm].numpy()
        if ref.ndim == 3:
            ref = ref[..., None]
        got = m1.tap(nm, 1, 32).cpu().numpy()
        e = rel_l2(got, ref)
        print(f"[tap bf16x3] {nm:10s} rel_l2={e:.3e}")
        assert e < 1e-3, nm
    _assert_parity(y, y_ref, "bf16x3 miso1 T=32 vs oracle")
    _assert_parity(y, g["y"], "bf16x3 miso1 T=32 vs reference golden")


@pytest.mark.parametrize("B,T", [(1, 96), (2, 130), (3, 40), (1, 5), (1, 128), (2, 257)])
def test_bf16x3_forward_shapes(nets_bf, sd1, B, T):
    from oracle import miso_oracle
    m1, _ = nets_bf
    r = np.random.default_rng(77 + T)
    x = (r.standard_normal((B, 6, T, 129)) + 1j * r.standard_normal((B, 6, T, 129))).astype(np.complex64)
    y = m1(torch.from_numpy(x).cuda()).cpu().numpy()
    y_ref = np.concatenate([miso_oracle.miso1_forward(torch.from_numpy(x[b:b + 1]), sd1).numpy() for b in range(B)])
    _assert_parity(y, y_ref, f"bf16x3 miso1 B={B} T={T} vs oracle")


def test_bf16x3_pipeline_vs_golden(nets_bf):
    import misonet_amd as mz
    m1, m3 = nets_bf
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    g = golden("g6_pipeline_T64.npz")
    mx, cl = _utt_inputs(7, 64)
    out, extra = enh.enhance(torch.from_numpy(mx[None]).cuda(), torch.from_numpy(cl[None]).cuda(), want_bf=True)
    _assert_parity(extra["bf"][0].cpu().numpy(), g["bf"], "bf16x3 pipeline bf vs golden")
    _assert_parity(out[0].cpu().numpy(), g["out"], "bf16x3 pipeline miso3 vs golden")


def test_bf16x3_full_size(nets_bf, sd1):
    from oracle import miso_oracle
    m1, _ = nets_bf
    mx, _ = _utt_inputs(1, 1001)
    y = m1(torch.from_numpy(mx[None]).cuda()).cpu().numpy()
    y_ref = miso_oracle.miso1_forward(torch.from_numpy(mx[None]), sd1).numpy()
    _assert_parity(y, y_ref, "bf16x3 miso1 T=1001 vs oracle")


def test_bf16x3_miso3_vs_golden(nets_bf):
    """MISO_3 (16 input channels: mix, beamformed, MISO1 estimate) against the reference golden G3."""
    _, m3 = nets_bf
    g = golden("g3_miso3_T32.npz")
    y = m3(torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["a"]).cuda(),
           torch.from_numpy(g["b"]).cuda()).cpu().numpy()
    _assert_parity(y, g["y"], "bf16x3 miso3 T=32 vs reference golden")


def test_bf16x3_config1_sample_clean_8khz(nets_bf):
    """BASELINE.json configs[0] (8 kHz, T = 501) against the golden produced by the real reference (G8)."""
    from oracle import pipeline_oracle
    m1, _ = nets_bf
    g = golden("g8_sample_clean_miso1.npz")
    x = pipeline_oracle.stft_chunk(g["obs_wav_f16"].astype(np.float32), 8000)[None]
    y = m1(torch.from_numpy(x).cuda()).cpu().numpy()
    assert y.shape == (1, 2, 501, 129)
    _assert_parity(y[:, :, 200:232], g["y_slice"], "bf16x3 config-1 sample/Clean slice vs reference golden")
    assert rel_l2(np.abs(y).sum(-1), g["mag_sum_per_frame"]) < 3e-4


def test_bf16x3_batch_invariance_and_repeatability(nets_bf):
    """Size-independent properties at the BASELINE geometry (T = 1001): a sample's result does not depend on the batch it
    runs in nor on its position (9 samples: one XCD's tile list holds two of them), and two runs are identical -- BIT FOR
    BIT: the instance-norm / gLN statistics are accumulated exactly (csrc/det_stats.hpp), there is no other run-to-run
    freedom."""
    m1, _ = nets_bf
    mx, _ = _utt_inputs(1, 1001)
    x = torch.from_numpy(mx[None]).cuda()
    y1 = m1(x).cpu().numpy()
    xb = torch.cat([x * (1.0 + 0.25 * i) for i in range(8)] + [x], dim=0)
    yb = m1(xb).cpu().numpy()
    # (any 1-ulp difference in a layer's statistics re-draws the bf16 rounding of the next layer's weights and shows up
    # as ~2e-5 here: this caught a sum of squares that was fused in one code path and not in another)
    assert np.array_equal(yb[8], y1[0])
    assert np.array_equal(yb[0], y1[0])
    yb2 = m1(xb).cpu().numpy()
    assert np.array_equal(yb2, yb)


def test_bf16x3_pipeline_batch_invariance(nets_bf):
    """The whole MISO1 -> PIT -> MVDR -> MISO3 path on 9 utterances (54 + 18 network samples: every XCD's tile list holds
    several) equals the same utterances run one by one, beamformer output and enhanced spectrogram alike."""
    import misonet_amd as mz
    m1, m3 = nets_bf
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    utts = [_utt_inputs(3 + (i % 3), 130) for i in range(9)]
    mx = torch.from_numpy(np.stack([u[0] for u in utts])).cuda()
    cl = torch.from_numpy(np.stack([u[1] for u in utts])).cuda()
    out_b, ex_b = enh.enhance(mx, cl, want_bf=True)
    out_b, bf_b = out_b.cpu().numpy(), ex_b["bf"].cpu().numpy()
    for i in (0, 4, 8):
        out_1, ex_1 = enh.enhance(mx[i:i + 1], cl[i:i + 1], want_bf=True)
        assert np.array_equal(bf_b[i], ex_1["bf"][0].cpu().numpy()), i
        assert np.array_equal(out_b[i], out_1[0].cpu().numpy()), i
    out_b2, ex_b2 = enh.enhance(mx, cl, want_bf=True)                      # run to run, the whole pipeline
    assert np.array_equal(out_b2.cpu().numpy(), out_b) and np.array_equal(ex_b2["bf"].cpu().numpy(), bf_b)


def test_bf16x3_long_utterance(nets_bf, sd1):
    """8 s at 16 kHz (T = 2001: 16 frame tiles per row, twice the BASELINE geometry) against the oracle."""
    from oracle import miso_oracle
    m1, _ = nets_bf
    mx, _ = _utt_inputs(2, 2001)
    y = m1(torch.from_numpy(mx[None]).cuda()).cpu().numpy()
    y_ref = miso_oracle.miso1_forward(torch.from_numpy(mx[None]), sd1).numpy()
    _assert_parity(y, y_ref, "bf16x3 miso1 T=2001 vs oracle")
