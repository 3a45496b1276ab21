"""Every choice of steps 4b and 5 of the fused pass (csrc/api_pipeline.hip, pipeline_run_impl) against its own stages, bit for bit, at
the geometries of tests/test_gpu_pipeline_glue.py: 1-4 speakers, 2-8 microphones, odd M, S = M, B = 3, Tp > T.

The fused-pass tests of the step-5 features (test_gpu_beamform, test_gpu_wpd, test_gpu_cacgmm, test_gpu_jbf) share one geometry,
S = 2, M = 6, ref_ch = 0, B = 2, at which a wrong index in the read path of those steps (kernels.hpp, src_row in pipeline mode:
n = b*M + m, sel[n*S + spk], the imaginary plane at (S + q) * plane) or in the image view of step 4b is hard or impossible to see
(tests/test_pipeline_glue.py, test_planted_read_faults_and_what_two_speakers_cannot_see).  Here, for every geometry and every
step-5 option, with refine off, guided and per bin:

    miso1      = the default configuration's miso1 (the raw estimate never moves)
    src        = miso1, or with refine refined_images(miso1, mix) = cacgmm(mix, masks_from_estimates(miso1, mix)) images
    bf         = Apply_Beamforming(src[:, j], mix, beamformer=spec) per speaker, or Apply_Beamforming_Joint(src, mix, jb)
    out        = MISO_3(mix, bf[b, j], miso1[b, j, ref_ch]) over the samples b*S + j: the RAW estimate, with refine on as well
    beamform_chunks() = bf, separate() = miso1

and: one handle walked through the options equals fresh handles (bits and workspace size); a workspace of 0xFF bytes and one of zeros
give the same bits with the refine regions and the larger step-5 blocks in play; WPD at its largest order; the refusal of the joint
kinds for S > M; the waveform entry and a captured graph.  Every comparison is equality of bits: there is no tolerance in this module.
Equal zeros or two untouched buffers cannot pass: every tensor is finite, every configuration's bf differs from the default's and
from the same step 5 without refine, and the drop-in calls report no failed bin (``diag_load = 1e-6`` is there for that; a case that
misses it gets another input or weight seed, never a relaxed condition).  No CPU network runs; the CPU work is NumPy gathers.
Figures: LAB.md, "Fused pass on its own stages"."""
import ctypes as C

import numpy as np
import pytest
import torch

import pipeline_glue_ref as G
from test_gpu_parity import _need_gpu
from test_gpu_pipeline_glue import CASES, F, _id, _networks, _same, _stages      # (_stages: mix_of, forced_orders, forced_clean)

pytestmark = pytest.mark.gpu

# (S, M, ref_ch, B, T, forced clean alignment): the glue module's cases in the library's default arithmetic, so networks, seeds and
# forced clean orders are shared
GEOMS = [c for c in CASES if c[6] is None and c[:5] in ((3, 6, 5, 2, 65), (4, 8, 2, 2, 33), (3, 5, 1, 2, 65), (4, 7, 6, 1, 33),
                                                       (2, 2, 1, 3, 65), (1, 3, 2, 2, 33))]
assert len(GEOMS) == 6
SWITCH_GEOM = next(c for c in GEOMS if c[:5] == (3, 5, 1, 2, 65))
WS_GEOM = next(c for c in GEOMS if c[:5] == (4, 8, 2, 2, 33))
REFUSAL_GEOM = (3, 2, 1, 2, 33, True, None)         # the pipeline admits S > M; the joint beamformers do not

STEP5_IDS = ["mvdr", "mpdr", "souden", "gev-ban", "wpd", "lcmv", "mwf", "r1mwf"]
REFINE = [None, dict(iterations=2, prior="guided"), dict(iterations=2, prior="bin")]


def _rid(rf):
    return "off" if rf is None else rf["prior"]


def step5(name, M):
    """the option of step 5; its own reference microphone is M - 1, deliberately not the pipeline's ref_ch"""
    from misonet_amd import Beamformer, JointBeamformer
    r = M - 1
    return {"mvdr": Beamformer(),
            "mpdr": dict(kind="mvdr", noise="mix"),
            "souden": dict(kind="souden", ref_ch=r),
            "gev-ban": dict(kind="gev", ban=True, ref_ch=r),
            "wpd": dict(kind="wpd", taps=3, delay=2, diag_load=1e-6, ref_ch=r),
            "lcmv": JointBeamformer(kind="lcmv", diag_load=1e-6, ref_ch=r),
            "mwf": JointBeamformer(kind="mwf", mu=1.0, diag_load=1e-6, ref_ch=r),
            "r1mwf": JointBeamformer(kind="r1mwf", mu=0.5, diag_load=1e-6, ref_ch=r)}[name]


def _finite(x):
    return bool(torch.isfinite(torch.view_as_real(x) if x.is_complex() else x).all())


def _run(enh, mix, clean):
    out, ex = enh.enhance(mix, clean, want_bf=True, want_miso1=True)
    return dict(out=out, bf=ex["bf"], miso1=ex["miso1"])


def drop_in(spec, src, mix_bf):
    """step 5 as the drop-in call on contiguous tensors: src [B, S, F, M, T], mix_bf [B, F, M, T] -> (bf [B, S, T, F], the number of
    failed bins the call reports, or None where the kind has no such flag)"""
    from misonet_amd import Apply_Beamforming, Apply_Beamforming_Joint, Beamformer, JointBeamformer
    if isinstance(spec, JointBeamformer):
        bf, dbg = Apply_Beamforming_Joint(src, mix_bf, spec, return_debug=True)
        return bf, int(dbg["fail"].sum())
    wpd = Beamformer.of(spec).kind == "wpd"
    cols, bad = [], 0 if wpd else None
    for j in range(src.shape[1]):
        if wpd:
            o, dbg = Apply_Beamforming(src[:, j], mix_bf, beamformer=spec, return_debug=True)
            bad += int(dbg["fail"].sum())
        else:
            o = Apply_Beamforming(src[:, j], mix_bf, beamformer=spec)
        cols.append(o)
    return torch.stack(cols, dim=1), bad


def miso3_of(m3, mix, bf, miso1, ref_ch):
    """MISO_3(mix, bf[b, j], miso1[b, j, ref_ch]) over the samples b*S + j"""
    B, S, M, T, _ = miso1.shape
    mix_rep = mix[:, None].expand(B, S, M, T, F).reshape(B * S, M, T, F)
    return m3(mix_rep, bf.reshape(B * S, 1, T, F), miso1[:, :, ref_ch].reshape(B * S, 1, T, F)).reshape(B, S, T, F)


_base = {}


def base_of(case):
    """what every test of a geometry shares, computed once and left unchanged: the networks, the input, the raw MISO_1 outputs, the
    forced clean references, the default configuration's results, and per refine option the refined images of its miso1"""
    from misonet_amd.refine import cacgmm, masks_from_estimates, refined_images
    key = case[:6]
    _networks(case[0], case[1], None)        # (another module may have left the shared networks in another arithmetic mode)
    if key not in _base:
        S, M, ref_ch, B, T, with_clean, _ = case
        m1, m3, enh, mix, raw, clean, c = _stages(case)
        d = _run(enh, mix, clean)
        assert all(_finite(v) for v in d.values()), _id(case)
        mix_bf = mix.permute(0, 3, 1, 2)                                                  # [B, F, M, T]
        est = d["miso1"].permute(0, 1, 4, 2, 3)                                           # [B, S, F, M, T]
        src, cfail = {"off": est}, {}
        for rf in REFINE[1:]:
            src[_rid(rf)] = refined_images(est, mix_bf, rf)
            # the same composition spelled out, with the diagnostics: no bin may have kept its initial masks
            _, img, dbg = cacgmm(mix_bf, masks_from_estimates(est, mix_bf), return_images=True, return_debug=True, refine=rf)
            assert _same(img, src[_rid(rf)]), f"{_id(case)}: refined_images is not cacgmm(masks_from_estimates) for {rf}"
            cfail[_rid(rf)] = int(dbg["fail"].sum())
            assert _finite(img) and not _same(img, est)
        _base[key] = dict(m1=m1, m3=m3, mix=mix, raw=raw, clean=clean, c=c, default=d, mix_bf=mix_bf, src=src, cfail=cfail)
    return _base[key]


# ---- 1. every configuration against the drop-in composition ------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEP5_IDS)
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_every_choice_equals_the_drop_in_composition(case, name):
    _need_gpu()
    import misonet_amd as mz
    S, M, ref_ch, B, T, with_clean, _ = case
    k = base_of(case)
    m1, m3, mix, clean, mix_bf, d0 = k["m1"], k["m3"], k["mix"], k["clean"], k["mix_bf"], k["default"]
    spec = step5(name, M)
    enh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch, beamformer=spec)
    bf_off, fails = None, []
    for rf in REFINE:
        what = f"{_id(case)} {name} refine {_rid(rf)}"
        enh.set_refine(rf)
        d = _run(enh, mix, clean)
        assert tuple(d["out"].shape) == (B, S, T, F) and tuple(d["bf"].shape) == (B, S, T, F)
        assert all(_finite(v) for v in d.values()), f"{what}: non-finite result"
        assert _same(d["miso1"], d0["miso1"]), f"{what}: miso1 is not the raw estimate of the default configuration"
        if rf is not None:
            assert k["cfail"][_rid(rf)] == 0, f"{what}: cacgmm reports {k['cfail'][_rid(rf)]} failed bins"
        want, bad = drop_in(spec, k["src"][_rid(rf)], mix_bf)
        fails.append(bad)
        assert bad is None or bad == 0, f"{what}: the drop-in call reports {bad} failed bins: another input or weight seed"
        assert _finite(want)
        assert _same(d["bf"], want), (f"{what}: step 5 of the fused pass differs from the drop-in call on "
                                      f"{'miso1' if rf is None else 'the refined images of miso1'}")
        assert _same(d["out"], miso3_of(m3, mix, d["bf"], d["miso1"], ref_ch)), \
            f"{what}: out is not MISO_3(mix, bf, the RAW miso1 at ref_ch)"
        assert _same(enh.beamform_chunks(mix, clean), d["bf"]), f"{what}: beamform_chunks() differs from the fused pass's bf"
        assert _same(enh.separate(mix, clean), d["miso1"]), f"{what}: separate() differs from the fused pass's miso1"
        # content: neither the default's numbers nor, with refine, the ones without it
        if name != "mvdr" or rf is not None:
            assert not _same(d["bf"], d0["bf"]) and not _same(d["out"], d0["out"]), f"{what}: the bits of the default configuration"
        else:
            assert _same(d["bf"], d0["bf"]) and _same(d["out"], d0["out"]), f"{what}: the defaults, set explicitly, differ"
        if rf is None:
            bf_off = d["bf"].clone()
        else:
            assert not _same(d["bf"], bf_off), f"{what}: refine leaves bf unchanged"
    print(f"[steps] {_id(case)} {name}: cacgmm fail {k['cfail']}, drop-in fail (off, guided, bin) {fails}")


# ---- 2. the cases can see the faults they are there for ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", GEOMS, ids=_id)
def test_selection_of_the_case_tells_the_planted_read_faults_apart(case):
    """on the case's OWN observed selection: the healthy read of src_row is the exported miso1, and every variant of
    pipeline_glue_ref.READ_FAULTS that this (S, B) can see changes what steps 4b and 5 would read"""
    _need_gpu()
    S, M, ref_ch, B, T, with_clean, _ = case
    k = base_of(case)
    raw_h, miso1_h = k["raw"].cpu().numpy(), k["default"]["miso1"].cpu().numpy()
    obs = G.observed_sel(miso1_h, raw_h, M)
    healthy = G.read_est(raw_h, obs, M, S)
    assert np.array_equal(G._bits(healthy), G._bits(G.gather(raw_h, obs, M))) and np.array_equal(G._bits(healthy), G._bits(miso1_h))
    seen = {f: not np.array_equal(G.read_est(raw_h, obs, M, S, f), healthy) for f in G.READ_FAULTS}
    print(f"[steps-sel] {_id(case)}: observed {obs.tolist()}; told apart: {[f for f in seen if seen[f]]}; "
          f"cannot be at this (S, B): {[f for f in seen if not G.READ_FAULT_NEEDS[f](S, B)]}")
    for f in G.READ_FAULTS:
        if G.READ_FAULT_NEEDS[f](S, B):
            assert seen[f], f"{_id(case)}: the selection {obs.tolist()} cannot see the planted fault {f!r} ({G.READ_FAULTS[f]})"
        else:
            assert not seen[f], (f, S, B)
    if S >= 3:
        e = G.expected(raw_h, k["clean"].cpu().numpy() if with_clean else None, M, S, ref_ch)
        cov = G.coverage(e["sel_shift"], e["sel_clean"])
        assert cov["non_involutive"] > 0, f"{_id(case)}: every shift permutation is its own inverse: {e['sel_shift'].tolist()}"


# ---- 3. switching on one handle leaves nothing behind ------------------------------------------------------------------------------
WALK = [("lcmv", None), ("lcmv", REFINE[1]), ("wpd", REFINE[1]), ("wpd", None), ("gev-ban", None), ("r1mwf", REFINE[2]),
        ("mvdr", None)]


def test_switching_on_one_handle_equals_fresh_handles():
    """both directions of every transition between the default, per-speaker, WPD and joint options, refine on and off: a stale
    use_wpd / use_joint / use_refine, or an offset of pipe_layout that did not move with them, shows in the bits or in the size"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import _lib
    case = SWITCH_GEOM
    S, M, ref_ch, B, T, _, _ = case
    k = base_of(case)
    m1, m3, mix, clean = k["m1"], k["m3"], k["mix"], k["clean"]
    nbytes = _lib.lib().misonet_pipeline_workspace_bytes
    enh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch)
    sizes = []
    for name, rf in WALK:
        what = f"{_id(case)} walk -> {name} refine {_rid(rf)}"
        spec = None if name == "mvdr" else step5(name, M)
        enh.set_beamformer(spec)
        enh.set_refine(rf)
        got = _run(enh, mix, clean)
        fresh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch, beamformer=spec, refine=rf)
        want = _run(fresh, mix, clean)
        for key in want:
            assert _finite(got[key]), f"{what}: non-finite {key}"
            assert _same(got[key], want[key]), f"{what}: {key} differs from a fresh Enhancer built in that configuration"
        n = nbytes(fresh._pipe, B, T)
        assert n > 0 and nbytes(enh._pipe, B, T) == n, (what, nbytes(enh._pipe, B, T), n)
        assert enh.workspace(B, T).numel() == n and fresh.workspace(B, T).numel() == n, what
        sizes.append(n)
    for key in want:                                                      # the walk ends where the shared default run started
        assert _same(got[key], k["default"][key]), f"{_id(case)}: back at the defaults, {key} differs from before"
    print(f"[steps-walk] {_id(case)}: workspace bytes {list(zip([f'{a}+{_rid(b)}' for a, b in WALK], sizes))}")
    assert sizes[1] > sizes[0] and sizes[2] > sizes[3] and sizes[5] > sizes[6]      # the refine block is there only when set


# ---- 4. the workspace's previous contents with the new regions in play; WPD at its largest order -----------------------------------
@pytest.mark.parametrize("name, rf", [("wpd", REFINE[1]), ("lcmv", REFINE[1]), ("mwf", REFINE[2])],
                         ids=["wpd+guided", "lcmv+guided", "mwf+bin"])
def test_workspace_previous_contents_do_not_matter_with_refine(name, rf):
    """rmask0, rmask, rimg, rws and the larger off_mvdr blocks: everything a pass reads of them it has written itself (cacgmm_bin_k
    writes the zeros of [T, Tp) too), so the workspace may hold anything before a pass"""
    _need_gpu()
    import misonet_amd as mz
    case = WS_GEOM
    S, M, ref_ch, B, T, _, _ = case
    k = base_of(case)
    enh = mz.Enhancer(k["m1"], k["m3"], num_spks=S, ref_ch=ref_ch, beamformer=step5(name, M), refine=rf)
    res = {}
    for byte in (0xFF, 0x00):
        ws = enh.workspace(B, T)
        ws.fill_(byte)
        res[byte] = {key: v.clone() for key, v in _run(enh, k["mix"], k["clean"]).items()}
        assert enh.workspace(B, T).data_ptr() == ws.data_ptr()
    for key in res[0]:
        assert _finite(res[0xFF][key]), f"{name}: non-finite {key} after a workspace of 0xFF bytes"
        assert _same(res[0xFF][key], res[0][key]), f"{name}: {key}: a workspace of 0xFF bytes and one of zeros give different bits"
    assert not _same(res[0]["bf"], k["default"]["bf"])


def test_wpd_at_the_largest_admitted_order():
    """M = 8, taps = 10: M (taps + 1) = 88 = WPD_KMAX, the largest stacked order the kernel takes, through the pipeline's views"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd.beamform import WPD_KMAX
    case = WS_GEOM
    S, M, ref_ch, B, T, _, _ = case
    assert M * (10 + 1) == WPD_KMAX
    k = base_of(case)
    spec = dict(kind="wpd", taps=10, delay=2, diag_load=1e-6, ref_ch=M - 1)
    enh = mz.Enhancer(k["m1"], k["m3"], num_spks=S, ref_ch=ref_ch, beamformer=spec)
    d = _run(enh, k["mix"], k["clean"])
    want, bad = drop_in(spec, k["src"]["off"], k["mix_bf"])
    print(f"[steps] {_id(case)} wpd taps 10: drop-in fail {bad}")
    assert all(_finite(v) for v in d.values()) and _finite(want)
    # (T = 33 frames against an order of 88: R has rank <= 33 before diag_load 1e-6 tr(R) / K, which is what makes it definite)
    assert bad == 0, f"the drop-in call reports {bad} failed bins"
    assert _same(d["miso1"], k["default"]["miso1"])
    assert _same(d["bf"], want), "WPD at order 88 in the fused pass differs from the drop-in call"
    assert _same(d["out"], miso3_of(k["m3"], k["mix"], d["bf"], d["miso1"], ref_ch))
    assert not _same(d["bf"], k["default"]["bf"])


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_joint_beamformers_are_refused_for_more_speakers_than_microphones():
    """S = 3, M = 2: misonet_pipeline_create admits it, jbf_opts_check does not; the refusal leaves the handle as it was, and refine
    (K = 4 classes on two microphones) is still taken"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import JointBeamformer, _lib
    case = REFUSAL_GEOM
    S, M, ref_ch, B, T, _, _ = case
    m1, m3, enh, mix, raw, clean, c = _stages(case)
    mix_bf = mix.permute(0, 3, 1, 2)
    d0 = _run(enh, mix, clean)
    assert all(_finite(v) for v in d0.values())
    with pytest.raises(ValueError):
        mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch, beamformer=JointBeamformer())
    with pytest.raises(ValueError):
        enh.set_beamformer(JointBeamformer(kind="mwf"))
    for jb in (JointBeamformer(), JointBeamformer(kind="mwf"), JointBeamformer(kind="r1mwf", mu=0.5)):
        opts = jb.c_opts()
        assert _lib.lib().misonet_pipeline_set_joint(enh._pipe, C.byref(opts)) == _lib.EINVAL, jb
    n0 = _lib.lib().misonet_pipeline_workspace_bytes(enh._pipe, B, T)
    d1 = _run(enh, mix, clean)
    for key in d0:
        assert _same(d1[key], d0[key]), f"{_id(case)}: {key} moved after a refused set_joint"
    # refine is accepted there and matches the drop-in composition
    from misonet_amd.refine import cacgmm, masks_from_estimates
    for rf in REFINE[1:]:
        enh.set_refine(rf)
        d = _run(enh, mix, clean)
        assert all(_finite(v) for v in d.values())
        assert _same(d["miso1"], d0["miso1"])
        est = d["miso1"].permute(0, 1, 4, 2, 3)
        _, img, dbg = cacgmm(mix_bf, masks_from_estimates(est, mix_bf), return_images=True, return_debug=True, refine=rf)
        assert int(dbg["fail"].sum()) == 0, (rf, int(dbg["fail"].sum()))
        want, _ = drop_in(mz.Beamformer(), img, mix_bf)
        assert _same(d["bf"], want), f"{_id(case)} refine {_rid(rf)}: bf differs from Apply_Beamforming on the refined images"
        assert _same(d["out"], miso3_of(m3, mix, d["bf"], d["miso1"], ref_ch))
        assert not _same(d["bf"], d0["bf"])
    enh.set_refine(None)
    assert _lib.lib().misonet_pipeline_workspace_bytes(enh._pipe, B, T) == n0
    d2 = _run(enh, mix, clean)
    for key in d0:
        assert _same(d2[key], d0[key]), f"{_id(case)}: {key} moved after refine was set and unset"


# ---- 6. one waveform entry and one captured graph ----------------------------------------------------------------------------------
def test_waveform_entry_and_captured_graph_with_lcmv_and_guided_refine():
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd.stft import stft_hip
    case = SWITCH_GEOM
    S, M, ref_ch, B, T, _, _ = case
    k = base_of(case)
    m1, m3, mix, clean = k["m1"], k["m3"], k["mix"], k["clean"]
    enh = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch, beamformer=step5("lcmv", M), refine=REFINE[1])
    # stft_pack_k straight into the layout against stft_hip + pack_k, with steps 4b and 5 reading what it packed
    n = 64 * (T - 1) + 17
    r = np.random.default_rng(9800 + M)
    wav = torch.from_numpy((0.1 * r.standard_normal((B, n, M))).astype(np.float32)).cuda()
    wav[1:] *= 3.0
    clean_wav = torch.from_numpy((0.1 * r.standard_normal((B, n, S))).astype(np.float32)).cuda()
    out_w, ex_w = enh.enhance_wav(wav, clean_wav, want_bf=True, want_miso1=True)
    smix, sclean = stft_hip(wav), stft_hip(clean_wav)
    assert tuple(smix.shape) == (B, M, T, F) and tuple(sclean.shape) == (B, S, T, F)
    out_s, ex_s = enh.enhance(smix, sclean, want_bf=True, want_miso1=True)
    for key, a, b in (("out", out_w, out_s), ("bf", ex_w["bf"], ex_s["bf"]), ("miso1", ex_w["miso1"], ex_s["miso1"])):
        assert _finite(a), (_id(case), key)
        assert _same(a, b), f"{_id(case)}: {key} from the waveform entry differs from the spectrogram entry"
    plain = mz.Enhancer(m1, m3, num_spks=S, ref_ch=ref_ch)
    assert not _same(ex_w["bf"], plain.enhance_wav(wav, clean_wav, want_bf=True)[1]["bf"])
    # a captured graph replays the bits of the eager pass
    eager = _run(enh, mix, clean)
    cp = enh.capture_graph(mix, clean)
    cp.out.zero_()
    cp.graph.replay()
    torch.cuda.synchronize()
    cp.check()
    assert _finite(cp.out) and _same(cp.out, eager["out"]), f"{_id(case)}: the captured graph does not replay the eager pass"
    assert not _same(cp.out, k["default"]["out"])
    del cp
