"""The selectable beamformers on the device (csrc/mvdr.hip: mvdr_scm_eig / bf_scm, mvdr_solve_ext, bf_solve) against the
float64 restatement tests/beamform_ref.py, and the layers above them: the defaults bit for bit, the fused pass, batch invariance, the Tester_Beamforming files and the edges.

Inputs carry a dominant rank-1 source (beamform_ref.rank1_inputs): on white inputs the principal eigenvalue gap falls to
about 1 % and the float32 covariance accumulation alone moves the float64 answer by 8e-5 at (1, 129, 6, 300).  On these inputs
the same CPU experiment (beamform_parts with the covariances accumulated in complex64 against complex128, NumPy's summation
order) moves out and w by <= 6.1e-6 over the four small shapes and by 1.1e-5 at (3, 129, 6, 1001), for every kind and option
set below, so the bar of the existing MVDR test, rel-L2 < 1e-4, sits an order of magnitude over the floor of the number
format and is not taken from what the kernels give.  T >= 2 M everywhere: with T < M the
result is set by eps.
Stage by stage (eig, phase, solve, apply at K = 4 float32 yardsticks), odd M and the frame-loop seams: tests/test_gpu_beamform_stages.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import beamform_ref as R
from conftest import golden, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-4
SMALL = [(2, 17, 4, 50), (1, 129, 6, 300), (1, 9, 2, 7), (1, 5, 8, 33)]
BIG = (3, 129, 6, 1001)
OPTS = [dict(beamformer=k, noise=n) for k in R.KINDS for n in ("residual", "mix")] + [
    dict(beamformer="gev", ban=True),
    dict(beamformer="gev", noise="mix", condition=1e-3, trace_normalize=True, ban=True),
    dict(beamformer="mvdr", condition=1e-3, trace_normalize=True, ban=True),
    dict(beamformer="souden", ref_ch=1)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_INPUTS = {}


def _inputs(shape):
    """(src, mix) complex64 ndarrays and their device copies, made once per shape and never written"""
    if shape not in _INPUTS:
        src, mix = R.rank1_inputs(*shape)
        _INPUTS[shape] = (src, mix, torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda())
    return _INPUTS[shape]


def _ref(src, mix, o):
    return R.beamform_parts(src, mix, kind=o["beamformer"], noise=o.get("noise", "residual"), condition=o.get("condition", 0.0),
                            trace_normalize=o.get("trace_normalize", False), ban_=o.get("ban", False), ref_ch=o.get("ref_ch", 0))


def _tag(o):
    return "+".join(f"{k}={v}" if k != "beamformer" else str(v) for k, v in o.items())


def _compare(shape, o):
    from misonet_amd import Apply_Beamforming
    src, mix, s_dev, m_dev = _inputs(shape)
    want = _ref(src, mix, o)
    out, dbg = Apply_Beamforming(s_dev, m_dev, return_debug=True, **o)
    e_o, e_w = rel_l2(out.cpu().numpy(), want["out"]), rel_l2(dbg["w"].cpu().numpy(), want["w"])
    print(f"[beamform] {_tag(o)} B,F,M,T={shape}: out {e_o:.3e} w {e_w:.3e}")
    assert tuple(out.shape) == (shape[0], shape[3], shape[1]) and out.dtype == torch.complex64
    assert e_o < TOL and e_w < TOL
    if o["beamformer"] == "gev":
        e_l = rel_l2(dbg["lam"].cpu().numpy(), want["lam"])
        print(f"[beamform]   lambda_max {e_l:.3e}")
        assert e_l < TOL
    else:
        assert "lam" not in dbg
    assert ("steer1" in dbg) == (o["beamformer"] == "mvdr")


@pytest.mark.parametrize("o", OPTS, ids=_tag)
@pytest.mark.parametrize("shape", SMALL, ids=str)
def test_kinds_and_options_vs_restatement(shape, o):
    _need_gpu()
    _compare(shape, o)


@pytest.mark.parametrize("kind", R.KINDS)
def test_full_size_vs_restatement(kind):
    _need_gpu()
    _compare(BIG, dict(beamformer=kind, ban=(kind == "gev")))


def _mvdr_direct(s_dev, m_dev, epsi=1e-6):
    from misonet_amd import _lib
    L = _lib.lib()
    B, F, M, T = s_dev.shape
    ws = torch.empty(L.misonet_mvdr_workspace_bytes(B, F, M), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, T, F), dtype=torch.complex64, device="cuda")
    _lib.check(L.misonet_mvdr(s_dev.data_ptr(), m_dev.data_ptr(), B, F, M, T, epsi, out.data_ptr(), ws.data_ptr(), ws.numel(),
                              _lib.stream_ptr(s_dev.device)))
    return out


def _beamform_direct(s_dev, m_dev, opts):
    from misonet_amd import _lib
    L = _lib.lib()
    B, F, M, T = s_dev.shape
    ws = torch.empty(L.misonet_beamform_workspace_bytes(B, F, M, C.byref(opts)), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, T, F), dtype=torch.complex64, device="cuda")
    _lib.check(L.misonet_beamform(s_dev.data_ptr(), m_dev.data_ptr(), B, F, M, T, C.byref(opts), out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr(s_dev.device)))
    return out


def test_defaults_are_bit_identical_to_misonet_mvdr():
    _need_gpu()
    from misonet_amd import Apply_Beamforming, _lib
    opts = _lib.BfOpts()
    _lib.lib().misonet_bf_opts_default(C.byref(opts))
    g = golden("g5_mvdr.npz")
    cases = [(torch.from_numpy(g["src"]).cuda(), torch.from_numpy(g["mix"]).cuda())]
    cases += [_inputs(shape)[2:] for shape in SMALL + [BIG]]
    for s_dev, m_dev in cases:
        want = _mvdr_direct(s_dev, m_dev)
        assert torch.equal(_beamform_direct(s_dev, m_dev, opts), want), tuple(s_dev.shape)
        assert torch.equal(Apply_Beamforming(s_dev, m_dev), want), tuple(s_dev.shape)
        assert torch.equal(Apply_Beamforming(s_dev, m_dev, 1e-6, beamformer="mvdr", noise="residual", condition=0.0,
                                             trace_normalize=False, ban=False, ref_ch=0), want), tuple(s_dev.shape)
    out, dbg = Apply_Beamforming(g["src"], g["mix"], return_debug=True)
    assert out.device.type == "cpu" and sorted(dbg) == ["steer1", "w"]
    assert rel_l2(out.numpy(), g["out"]) < TOL and rel_l2(dbg["w"].cpu().numpy(), g["w"]) < TOL


@pytest.mark.parametrize("kind", ["gev", "souden"])
def test_batch_invariance_bit_exact(kind):
    _need_gpu()
    from misonet_amd import Apply_Beamforming
    _, _, s_dev, m_dev = _inputs(BIG)
    o = dict(beamformer=kind, ban=True, noise="mix", condition=1e-3)
    all3, d3 = Apply_Beamforming(s_dev, m_dev, return_debug=True, **o)
    one, d1 = Apply_Beamforming(s_dev[1:2].contiguous(), m_dev[1:2].contiguous(), return_debug=True, **o)
    assert torch.equal(all3[1:2], one) and torch.equal(d3["w"][1:2], d1["w"])
    again = Apply_Beamforming(s_dev, m_dev, **o)
    assert torch.equal(again, all3)                        # and from run to run


@pytest.fixture(scope="module")
def nets(sd1, sd3):
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    return m1.eval(), m3.eval()


def _chunks(utts, frames):
    from misonet_amd.weights import synthetic_utterance
    from oracle import pipeline_oracle
    mixs, cleans = [], []
    for u in utts:
        obs, s0, s1 = synthetic_utterance(u, (frames - 1) * 64)
        mixs.append(pipeline_oracle.stft_chunk(obs))
        cleans.append(np.stack([pipeline_oracle.stft_chunk(s0)[0], pipeline_oracle.stft_chunk(s1)[0]]))
    return torch.from_numpy(np.stack(mixs)).cuda(), torch.from_numpy(np.stack(cleans)).cuda()


def test_fused_pass_takes_the_beamformer(nets):
    """B = 2, T = 96.  The fused pass and Apply_Beamforming run the same kernels on the same float32 values (the aligned MISO1
    planes, the mixture), in the same order: the beamformer output is expected bit for bit, no tolerance."""
    import misonet_amd as mz
    from misonet_amd import Apply_Beamforming
    m1, m3 = nets
    mix, clean = _chunks((7, 11), 96)
    bf = {"kind": "gev", "ban": True}
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0, beamformer=bf)
    out, ex = enh.enhance(mix, clean, want_bf=True, want_miso1=True)
    mix_bf = mix.permute(0, 3, 1, 2)
    for s in range(2):
        want = Apply_Beamforming(ex["miso1"][:, s].permute(0, 3, 1, 2), mix_bf, beamformer="gev", ban=True)
        assert torch.equal(ex["bf"][:, s], want), s
    plain = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out0, ex0 = plain.enhance(mix, clean, want_bf=True)
    assert not torch.equal(ex["bf"], ex0["bf"]) and not torch.equal(out, out0)
    assert rel_l2(out.cpu().numpy(), out0.cpu().numpy()) > 1e-3            # MISO3 saw another beamformer
    # set and reset: bit-identical to an Enhancer that never left the defaults
    enh.set_beamformer(None)
    out1, ex1 = enh.enhance(mix, clean, want_bf=True)
    assert torch.equal(out1, out0) and torch.equal(ex1["bf"], ex0["bf"])
    with pytest.raises(ValueError):
        enh.set_beamformer({"kind": "gev", "ref_ch": 6})
    with pytest.raises(ValueError):
        mz.Enhancer(m1, m3, beamformer={"kind": "lcmv"})
    # beamform_chunks of the same Enhancer follows the setting too
    enh.set_beamformer(bf)
    assert torch.equal(enh.beamform_chunks(mix, clean), ex["bf"])


@pytest.mark.parametrize("utterance_flag", [True, False])
def test_tester_beamforming_takes_the_beamformer(nets, tmp_path, utterance_flag):
    """a two-chunk recording through the harness class with ``beamformer`` set: the files are those of beamform_utterance /
    beamform_chunks called with the same options, byte for byte"""
    import misonet_amd as mz
    from misonet_amd import stft as S
    from misonet_amd.stft import split_chunks
    from misonet_amd.tester import Tester_Beamforming
    from misonet_amd.weights import synthetic_utterance
    from oracle import pipeline_oracle
    m1, _ = nets
    frames, gap = 48, 700
    chunk = (frames - 1) * 64
    obs, s0, s1 = synthetic_utterance(21, 2 * chunk - gap)
    parts = [split_chunks(x, chunk)[0] for x in (obs, s0, s1)]
    obs_d, s0_d, s1_d = ({str(k): torch.from_numpy(pipeline_oracle.stft_chunk(p))[None] for k, p in enumerate(ps)}
                         for ps in parts)
    item = (obs_d, s0_d, s1_d, [gap], ["rec"])
    bf = {"kind": "gev", "ban": True, "noise": "mix"}
    tst = Tester_Beamforming("SMS_WSJ", [item], [], [], m1, 6, 0, 2, chunk / 16000, str(tmp_path / "t"), 0, True, True,
                             utterance_flag, fs=16000, window="hann", length=256, overlap=192)
    tst.beamformer = bf
    wav = tst.test()["train_si284"]["rec"]
    enh = mz.Enhancer(m1, None, num_spks=2, ref_ch=0)
    obs_k = [obs_d[str(k)][0].cuda() for k in range(2)]
    cl_k = [torch.stack((s0_d[str(k)][0, 0], s1_d[str(k)][0, 0])).cuda() for k in range(2)]
    if utterance_flag:
        want = enh.beamform_utterance(obs_k, cl_k, gap, beamformer=bf)
        plain = enh.beamform_utterance(obs_k, cl_k, gap)
    else:
        pcm = [S.istft_int16(enh.beamform_chunks(obs_k[k][None], cl_k[k][None], beamformer=bf))[0].cpu().numpy() for k in range(2)]
        want = np.stack([S.stitch_int16([pcm[k][s] for k in range(2)], gap) for s in range(2)])
        plain = None
    assert np.array_equal(wav, want)
    if plain is not None:
        assert not np.array_equal(wav, plain)
    for s in range(2):
        p = str(tmp_path / f"want_{s}.wav")
        S.write_wav_pcm24(p, want[s], 16000)
        assert open(p, "rb").read() == open(str(tmp_path / "t" / "train_si284" / f"rec_{s}.wav"), "rb").read()
    # the attribute is read when inference starts: back to the defaults for the next run
    tst.beamformer = None
    again = tst.test()["train_si284"]["rec"]
    assert not np.array_equal(again, wav)


def test_edges():
    _need_gpu()
    from misonet_amd import Apply_Beamforming
    _, _, s_dev, m_dev = _inputs(SMALL[0])
    zero = torch.zeros_like(s_dev)
    for kind in ("mvdr", "gev"):
        assert bool(torch.isfinite(torch.view_as_real(Apply_Beamforming(zero, m_dev, beamformer=kind))).all()), kind
    out = Apply_Beamforming(zero, m_dev, beamformer="souden")
    assert torch.equal(out, torch.zeros_like(out))
    for bad in (dict(ref_ch=4), dict(beamformer="lcmv"), dict(condition=-1e-3)):
        with pytest.raises(ValueError):
            Apply_Beamforming(s_dev, m_dev, **bad)
