"""GPU tests of the joint multi-speaker beamformers (csrc/jbf.hip, ``Apply_Beamforming_Joint``, the fused pass with a
``JointBeamformer``) against the float64 NumPy restatement of tests/jbf_ref.py: output, weights and relative transfer functions
on every shape at which a path of the kernel changes (jbf_ref.SHAPES), for every kind, both ends of ref_ch, with and without
diagonal loading, both rtf rules and both noise models of lcmv, two values of mu; the constraint w_s^H d_j = delta_sj on the
device's own numbers; bit-reproducibility and independence of the batch; the failure rule; a workspace and an output full of
NaN; and the fused pass, its captured graph, the beamform_* methods and Tester_Beamforming against the drop-in call.

Bars.  Output: rel-L2 <= 2.4e-7 = 4 x 2^-24, the one complex64 rounding of a float64 result (as tests/wpd_ref.py derives it).
Weights and RTFs: rel-L2 <= max(100 x the restatement's route (a) - (b) difference on that case, 1e-12); the margin covers the
third summation order the device adds.  The constraint: max |w_s^H d_j - delta_sj| <= max(100 x the restatement's own residual
on that case, 1e-12).  tests/test_jbf.py asserts the conditions these rest on (route difference <= 1e-12, eigenvalue gap >= 2,
no failed bin) for every case used here, and that planted faults miss these bars.  The module prints every figure
(``[jbf] ...``); LAB.md has them."""
import ctypes as C

import numpy as np
import pytest
import torch

import jbf_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
KW0 = {"lcmv": dict(noise="residual", rtf="cw", diag_load=0.0, ref_ch=0), "mwf": dict(mu=1.0, diag_load=0.0, ref_ch=0),
       "r1mwf": dict(mu=0.0, diag_load=0.0, ref_ch=0)}


def _run(src, mix, kind, **kw):
    from misonet_amd import Apply_Beamforming_Joint
    out, dbg = Apply_Beamforming_Joint(torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda(), kind, return_debug=True, **kw)
    return dict(out=out.cpu().numpy(), w=dbg["w"].cpu().numpy(), rtf=dbg["rtf"].cpu().numpy() if "rtf" in dbg else None,
                fail=dbg["fail"].cpu().numpy())


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.complex64 else np.uint8)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("out", "w", "fail")) and \
        (a["rtf"] is None or np.array_equal(_bits(a["rtf"]), _bits(b["rtf"])))


def _constraint(w, d):
    S = w.shape[1]
    return float(np.max(np.abs(np.einsum("bsfm,bjfm->bfsj", np.conj(w), d) - np.eye(S))))


@pytest.mark.parametrize("shape", R.SHAPES, ids=["-".join(map(str, s)) for s in R.SHAPES])
@pytest.mark.parametrize("kind", R.KINDS)
def test_against_restatement(shape, kind):
    """every option set of the kind on the shape against route (a); for lcmv also the constraint on the device's own w and d"""
    _need_gpu()
    src, mix = R.inputs(shape)
    n = 0
    for k, kw in R.options(shape):
        if k != kind:
            continue
        n += 1
        want = R.case(shape, kind, kw)
        diff, bar_w = R.bars(shape, kind, kw)
        got = _run(src, mix, kind, **kw)
        e_out, e_w = R.rel(got["out"], want["out"]), R.rel(got["w"], want["w"])
        line = f"[jbf] {R.case_id(shape, kind, kw)}: out {e_out:.3e} (bar {R.OUT_BAR:g})  w {e_w:.3e}"
        e_d = res = bar_c = None
        if kind == "lcmv":
            e_d = R.rel(got["rtf"], want["rtf"])
            res, bar_c = _constraint(got["w"], got["rtf"]), max(100.0 * want["resid"], 1e-12)
            line += f"  rtf {e_d:.3e}"
        line += f" (routes {diff:.3e}, bar {bar_w:.3e})"
        if kind == "lcmv":
            line += f"  constraint {res:.3e} (restatement {want['resid']:.3e}, bar {bar_c:.3e})"
        print(line)
        assert got["out"].dtype == np.complex64 and got["out"].shape == want["out"].shape and got["w"].shape == want["w"].shape
        assert not want["fail"].any() and not got["fail"].any(), kw
        assert e_out <= R.OUT_BAR, (kw, e_out)
        assert e_w <= bar_w, (kw, e_w, bar_w)
        if kind == "lcmv":
            assert e_d <= bar_w, (kw, e_d, bar_w)
            assert res <= bar_c, (kw, res, bar_c)
        else:
            assert got["rtf"] is None
    assert n == (16 if kind == "lcmv" else 8)


@pytest.mark.parametrize("kind", R.KINDS)
def test_bit_reproducible_and_batch_independent(kind):
    _need_gpu()
    S, M, T, F = 2, 6, 129, 9
    src, mix = R.jbf_inputs(3, S, M, T, F)
    kw = dict(KW0[kind], diag_load=1e-6, ref_ch=1)
    a, b = _run(src, mix, kind, **kw), _run(src, mix, kind, **kw)
    assert _same(a, b) and not a["fail"].any()
    for i in range(3):
        one = _run(src[i:i + 1], mix[i:i + 1], kind, **kw)
        assert _same(one, {k: (v[i:i + 1] if v is not None else None) for k, v in a.items()}), i


@pytest.mark.parametrize("kind,mu", [("lcmv", 1.0), ("mwf", 1.0), ("r1mwf", 0.0), ("r1mwf", 1.0)])
def test_failure_rule(kind, mu):
    """an all-zero bin of mixture and sources, and an all-zero estimate of one speaker: lcmv fails the whole bin; mwf gives that
    speaker an exact zero without a flag and the other speaker its filter; r1mwf with mu = 0 flags that speaker.  The flags are
    the restatement's, every other bin is within the bars"""
    _need_gpu()
    shape = R.SHAPES[2]
    src, mix = (x.copy() for x in R.inputs(shape))
    src[0, :, 1] = 0
    mix[0, 1] = 0
    src[1, 1, 3] = 0
    kw = dict(KW0[kind])
    if kind != "lcmv":
        kw["mu"] = mu
    want = R.jbf(src, mix, kind, **kw)
    other = R.jbf(src, mix, kind, route="b", **kw)
    got = _run(src, mix, kind, **kw)
    assert np.array_equal(got["fail"], want["fail"]) and np.array_equal(other["fail"], want["fail"])
    assert got["fail"][0, :, 1].all() and not got["out"][0, :, :, 1].any() and not got["w"][0, :, 1].any()
    if kind == "lcmv":
        assert got["fail"][1, :, 3].all() and got["fail"].sum() == 4
        assert not got["out"][1, :, :, 3].any() and not got["w"][1, :, 3].any() and not got["rtf"][1, :, 3].any()
    else:
        assert got["fail"][1, 0, 3] == 0 and got["fail"][1, 1, 3] == (1 if kind == "r1mwf" and mu == 0.0 else 0)
        assert not got["out"][1, 1, :, 3].any() and not got["w"][1, 1, 3].any()      # exactly zero, flagged or not
        assert got["out"][1, 0, :, 3].any()
    ok = want["fail"] == 0
    assert np.isfinite(got["out"]).all() and np.isfinite(got["w"]).all()
    bar_w = max(100.0 * R.rel(other["w"], want["w"]), R.W_FLOOR)
    e_out, e_w = R.rel(got["out"], want["out"]), R.rel(got["w"][ok], want["w"][ok])
    print(f"[jbf] failure rule {kind} mu {mu:g}: out {e_out:.3e} (bar {R.OUT_BAR:g})  w {e_w:.3e} (bar {bar_w:.3e})")
    assert e_out <= R.OUT_BAR and e_w <= bar_w


@pytest.mark.parametrize("kind", R.KINDS)
def test_nan_workspace_and_output_change_nothing(kind):
    _need_gpu()
    from misonet_amd import _lib
    from misonet_amd.beamform import JointBeamformer
    shape = R.SHAPES[2]
    B, S, M, T, F = shape
    src, mix = (torch.from_numpy(x).cuda() for x in R.inputs(shape))
    L = _lib.lib()
    o = JointBeamformer(kind=kind, **KW0[kind]).c_opts()
    n = L.misonet_beamform_joint_workspace_bytes(B, S, F, M, C.byref(o))
    st = _lib.stream_ptr(mix.device)
    got = []
    for fill in (0.0, float("nan")):
        ws = torch.full((n // 8 + 1,), fill, dtype=torch.float64, device="cuda")
        out = torch.full((B, S, T, F), fill, dtype=torch.complex64, device="cuda")
        w = torch.empty((B, S, F, M), dtype=torch.complex128, device="cuda")
        d = torch.empty((B, S, F, M), dtype=torch.complex128, device="cuda") if kind == "lcmv" else None
        bad = torch.empty((B, S, F), dtype=torch.int32, device="cuda")
        _lib.check(L.misonet_beamform_joint(src.data_ptr(), mix.data_ptr(), B, S, F, M, T, C.byref(o), out.data_ptr(),
                                            ws.data_ptr(), n, st))
        _lib.check(L.misonet_beamform_joint_debug(ws.data_ptr(), B, S, F, M, C.byref(o), w.data_ptr(),
                                                  d.data_ptr() if d is not None else None, bad.data_ptr(), st))
        got.append(dict(out=out.cpu().numpy(), w=w.cpu().numpy(), rtf=d.cpu().numpy() if d is not None else None,
                        fail=bad.cpu().numpy()))
    assert np.isfinite(got[0]["out"]).all() and not got[0]["fail"].any()
    assert _same(got[0], got[1])
    # the library refuses a short workspace and more speakers than microphones with a device as it does without one
    assert L.misonet_beamform_joint(src.data_ptr(), mix.data_ptr(), B, S, F, M, T, C.byref(o), out.data_ptr(), ws.data_ptr(), n - 1,
                                    st) == _lib.ENOMEM
    assert L.misonet_beamform_joint(src.data_ptr(), mix.data_ptr(), B, M + 1, F, M, T, C.byref(o), out.data_ptr(), ws.data_ptr(),
                                    1 << 40, st) == _lib.EINVAL
    if kind != "lcmv":
        assert L.misonet_beamform_joint_debug(ws.data_ptr(), B, S, F, M, C.byref(o), None, w.data_ptr(), None, st) == _lib.EINVAL


def test_numpy_in_numpy_out():
    _need_gpu()
    from misonet_amd import Apply_Beamforming_Joint
    shape = R.SHAPES[1]
    src, mix = R.inputs(shape)
    out = Apply_Beamforming_Joint(src, mix)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.complex64
    assert R.rel(out.numpy(), R.case(shape, "lcmv", KW0["lcmv"])["out"]) <= R.OUT_BAR
    # permuted views are taken as they are
    s_dev = torch.from_numpy(np.ascontiguousarray(src.transpose(0, 1, 3, 4, 2))).cuda().permute(0, 1, 4, 2, 3)
    got = Apply_Beamforming_Joint(s_dev, torch.from_numpy(mix).cuda())
    assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(out.numpy()))


# ---- the fused pass ------------------------------------------------------------------------------------------------------
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


def _eq(a, b):
    return torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_fused_pass(nets):
    """step 5 of the fused pass is the drop-in call's kernel through other views: the same bits for lcmv and r1mwf; a captured
    graph replays them; set_beamformer(None) restores the bits and the workspace size of an Enhancer that never left the defaults;
    beamform_chunks honours the options; with refine set the step equals the drop-in on the refined images"""
    import misonet_amd as mz
    from misonet_amd import Apply_Beamforming_Joint, JointBeamformer, _lib
    from misonet_amd.refine import refined_images
    from test_gpu_beamform import _chunks
    m1, m3 = nets
    B, T = 2, 96
    mix, clean = _chunks((7, 11), T)
    mix_bf = mix.permute(0, 3, 1, 2)                                                         # [B, F, M, T]
    plain = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out0, d0 = plain.enhance(mix, clean, want_bf=True)
    n0 = _lib.lib().misonet_pipeline_workspace_bytes(plain._pipe, B, T)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    for jb in (JointBeamformer(kind="lcmv", diag_load=1e-6), JointBeamformer(kind="r1mwf", mu=0.5, ref_ch=1)):
        enh.set_beamformer(jb)
        assert enh.beamformer is jb
        out1, d1 = enh.enhance(mix, clean, want_bf=True, want_miso1=True)
        assert torch.isfinite(torch.view_as_real(d1["bf"])).all() and not _eq(d1["bf"], d0["bf"]) and not _eq(out1, out0)
        est = d1["miso1"].permute(0, 1, 4, 2, 3)                                             # [B, S, F, M, T]
        assert _eq(d1["bf"], Apply_Beamforming_Joint(est, mix_bf, jb)), jb
        assert _eq(enh.beamform_chunks(mix, clean), d1["bf"]), jb
        assert _eq(plain.beamform_chunks(mix, clean, beamformer=jb), d1["bf"]), jb
        # with refine set, step 5 reads the refined images
        rf = dict(iterations=2, prior="guided")
        enh.set_refine(rf)
        d2 = enh.enhance(mix, clean, want_bf=True)[1]
        assert _eq(d2["bf"], Apply_Beamforming_Joint(refined_images(est, mix_bf, rf), mix_bf, jb)), jb
        assert not _eq(d2["bf"], d1["bf"])
        enh.set_refine(None)
        # a captured graph replays the same bits, and refuses a change of the beamformer while it lives
        cp = enh.capture_graph(mix, clean)
        cp.out.zero_()
        cp.graph.replay()
        torch.cuda.synchronize()
        assert _eq(cp.out, out1), jb
        with pytest.raises(RuntimeError):
            enh.set_beamformer(None)
        with pytest.raises(RuntimeError):
            enh.set_beamformer(JointBeamformer(kind="mwf"))
        del cp
    # bad fields never reach the pipeline; a name or a dict still means Beamformer
    with pytest.raises(ValueError):
        enh.set_beamformer(JointBeamformer(kind="mwf", mu=0.0))
    with pytest.raises(ValueError):
        enh.set_beamformer(JointBeamformer(ref_ch=6))
    with pytest.raises(ValueError):
        enh.set_beamformer("lcmv")
    assert isinstance(enh.beamformer, JointBeamformer)
    # back: the bits and the workspace size of an Enhancer that never left the defaults
    enh.set_beamformer(None)
    out2, d2 = enh.enhance(mix, clean, want_bf=True)
    assert _eq(out2, out0) and _eq(d2["bf"], d0["bf"])
    assert _lib.lib().misonet_pipeline_workspace_bytes(enh._pipe, B, T) == n0
    # the constructor takes an instance too
    enh3 = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0, beamformer=JointBeamformer(kind="lcmv", diag_load=1e-6))
    jb0 = JointBeamformer(kind="lcmv", diag_load=1e-6)
    assert _eq(enh3.enhance(mix, clean, want_bf=True)[1]["bf"], plain.beamform_chunks(mix, clean, beamformer=jb0))


@pytest.mark.parametrize("utterance_flag", [True, False])
def test_tester_beamforming_takes_a_joint_beamformer(nets, tmp_path, utterance_flag):
    """a two-chunk recording through the harness class with ``beamformer`` a JointBeamformer: beamform_utterance is the
    composition with Apply_Beamforming_Joint, and the files are those of beamform_utterance / beamform_chunks, byte for byte"""
    import misonet_amd as mz
    from misonet_amd import Apply_Beamforming_Joint, JointBeamformer
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
    jb = JointBeamformer(kind="lcmv", noise="mix", diag_load=1e-6)
    tst = Tester_Beamforming("SMS_WSJ", [item], [], [], m1, 6, 0, 2, chunk / 16000, str(tmp_path / "t"), 0, True, True,
                             utterance_flag, fs=16000, window="hann", length=256, overlap=192)
    tst.beamformer = jb
    wav = tst.test()["train_si284"]["rec"]
    enh = mz.Enhancer(m1, None, num_spks=2, ref_ch=0)
    obs_k = [obs_d[str(k)][0].cuda() for k in range(2)]
    cl_k = [torch.stack((s0_d[str(k)][0, 0], s1_d[str(k)][0, 0])).cuda() for k in range(2)]
    if utterance_flag:
        want = enh.beamform_utterance(obs_k, cl_k, gap, beamformer=jb)
        # the same tail by hand: one joint call over the whole recording's frames
        est = enh.separate(torch.stack(obs_k), torch.stack(cl_k))
        e, o = S.istft(est), S.istft(torch.stack(obs_k))
        n = e.shape[-1]
        keep = [n, n - gap]
        est_t = torch.cat([e[k, ..., :keep[k]] for k in range(2)], dim=-1)
        obs_t = torch.cat([o[k, ..., :keep[k]] for k in range(2)], dim=-1)
        pad = (-obs_t.shape[-1]) % S.HOP
        sig = torch.nn.functional.pad(torch.cat([obs_t[None], est_t], dim=0), (0, pad)).permute(0, 2, 1).contiguous()
        spec = S.stft_hip(sig)
        bf = Apply_Beamforming_Joint(spec[1:].permute(0, 3, 1, 2)[None], spec[0].permute(2, 0, 1)[None], jb)[0]
        assert np.array_equal(want, S.istft_int16(bf).cpu().numpy())
        assert not np.array_equal(want, enh.beamform_utterance(obs_k, cl_k, gap))
    else:
        pcm = []
        for k in range(2):
            est = enh.separate(obs_k[k][None], cl_k[k][None]).permute(0, 1, 4, 2, 3)
            bf = Apply_Beamforming_Joint(est, obs_k[k][None].permute(0, 3, 1, 2), jb)
            assert _eq(bf, enh.beamform_chunks(obs_k[k][None], cl_k[k][None], beamformer=jb))
            pcm.append(S.istft_int16(bf)[0].cpu().numpy())
        want = np.stack([S.stitch_int16([pcm[k][s] for k in range(2)], gap) for s in range(2)])
    assert np.array_equal(wav, want)
    for s in range(2):
        p = str(tmp_path / f"want_{s}.wav")
        S.write_wav_pcm24(p, want[s], 16000)
        assert open(p, "rb").read() == open(str(tmp_path / "t" / "train_si284" / f"rec_{s}.wav"), "rb").read()
    # the attribute is read when inference starts: back to the defaults for the next run
    tst.beamformer = None
    assert not np.array_equal(tst.test()["train_si284"]["rec"], wav)
