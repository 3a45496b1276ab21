"""GPU tests of the WPD convolutional beamformer (csrc/wpd.hip, ``Apply_Beamforming(beamformer="wpd")``, the fused pass with
``Beamformer(kind="wpd")``) against the float64 NumPy restatement of tests/wpd_ref.py: output and weights on every shape that
takes another path (T below one tile, the smallest and the largest order, odd M, T no multiple of a tile), both ends of ref_ch,
with and without diagonal loading, a floor that binds; bit-reproducibility and independence of the batch; the failure rule; a
workspace full of NaN; and the fused pass, its captured graph and the beamform_* methods against the drop-in call.

Bars.  Output: rel-L2 <= 2.4e-7 = 4 x 2^-24 (one complex64 rounding of a float64 result is bounded by 2^-24 per element;
tests/test_wpd.py asserts that the float64 path's own sensitivity on these inputs is below 1e-10).  Weights wbar: 100 x the
LU-versus-Cholesky difference of the restatement's wbar on that case, never below 1e-12 (the margin covers the third summation
order the device adds).  The module prints every figure (``[wpd] ...``); LAB.md has them."""
import functools

import numpy as np
import pytest
import torch

import wpd_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _inputs(B, M, T, F):
    return R.wpd_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _ref(shape, ref_ch, diag_load, power_floor=1e-10):
    """(out, wbar, fail, LU-versus-Cholesky rel-L2 of wbar) of the restatement, computed once per case"""
    B, M, T, F, taps, delay = shape
    mix, src = _inputs(B, M, T, F)
    out, wb, bad, _ = R.wpd(src, mix, taps, delay, diag_load, power_floor, ref_ch)
    wc = R.wpd(src, mix, taps, delay, diag_load, power_floor, ref_ch, solver="chol")[1]
    return out, wb, bad, R.rel(wc, wb)


def _run(src, mix, **kw):
    from misonet_amd.beamform import Apply_Beamforming
    out, dbg = Apply_Beamforming(torch.from_numpy(src).cuda(), torch.from_numpy(mix).cuda(), beamformer="wpd",
                                 return_debug=True, **kw)
    return out.cpu().numpy(), dbg["w"].cpu().numpy(), dbg["fail"].cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.complex64 else np.uint8)


def _check(shape, ref_ch, diag_load, tag, power_floor=1e-10):
    B, M, T, F, taps, delay = shape
    want, wb, bad, lu_chol = _ref(shape, ref_ch, diag_load, power_floor)
    mix, src = _inputs(B, M, T, F)
    out, w, fail = _run(src, mix, taps=taps, delay=delay, diag_load=diag_load, power_floor=power_floor, ref_ch=ref_ch)
    e_out, e_w, bar_w = R.rel(out, want), R.rel(w, wb), max(100.0 * lu_chol, 1e-12)
    print(f"[wpd] {tag} {shape} ref {ref_ch} load {diag_load:g} floor {power_floor:g}: out {e_out:.3e} (bar {R.OUT_BAR:g})  "
          f"wbar {e_w:.3e} (LU vs Cholesky {lu_chol:.3e}, bar {bar_w:.3e})")
    assert out.dtype == np.complex64 and out.shape == want.shape and w.shape == wb.shape
    assert not bad.any() and not fail.any()
    assert e_out <= R.OUT_BAR, (tag, e_out)
    assert e_w <= bar_w, (tag, e_w, bar_w)


@pytest.mark.parametrize("diag_load", [0.0, 1e-6])
@pytest.mark.parametrize("last_ref", [False, True], ids=["ref0", "refM-1"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_restatement(shape, last_ref, diag_load):
    _need_gpu()
    _check(shape, shape[1] - 1 if last_ref else 0, diag_load, "case")


def test_floor_that_binds():
    """power_floor = 0.05 limits the weights of the quiet frames (tests/test_wpd.py: dropping the floor there misses the bars)"""
    _need_gpu()
    _check(R.SHAPES[2], 0, 0.0, "floor", power_floor=0.05)


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    B, M, T, F, taps, delay = 3, 4, 150, 9, 3, 2
    mix, src = _inputs(B, M, T, F)
    a = _run(src, mix, taps=taps, delay=delay)
    b = _run(src, mix, taps=taps, delay=delay)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert not a[2].any() and np.abs(a[0]).min() > 0
    for i in range(B):
        one = _run(np.ascontiguousarray(src[i:i + 1]), np.ascontiguousarray(mix[i:i + 1]), taps=taps, delay=delay)
        assert np.array_equal(_bits(a[0][i]), _bits(one[0][0])), i
        assert np.array_equal(_bits(a[1][i]), _bits(one[1][0])), i


def test_failure_rule():
    """an all-zero bin and an all-zero source estimate give out exactly 0 and fail = 1 there; the other bins stay in the bar"""
    _need_gpu()
    B, M, T, F, taps, delay = R.SHAPES[0]
    mix, src = (x.copy() for x in _inputs(B, M, T, F))
    mix[1, 4] = 0
    src[1, 4] = 0
    src[0, 2] = 0
    want, wb, bad, _ = R.wpd(src, mix, taps, delay)
    out, w, fail = _run(src, mix, taps=taps, delay=delay)
    flags = np.zeros((B, F), np.int32)
    flags[1, 4] = flags[0, 2] = 1
    assert np.array_equal(fail, flags) and np.array_equal(bad, flags)
    assert not _bits(out[1, :, 4]).any() and not _bits(out[0, :, 2]).any()
    assert not _bits(w[1, 4]).any() and not _bits(w[0, 2]).any()
    keep = flags == 0
    e = R.rel(out.transpose(0, 2, 1)[keep], want.transpose(0, 2, 1)[keep])
    print(f"[wpd] failure rule: the other bins {e:.3e}")
    assert e <= R.OUT_BAR and R.rel(w[keep], wb[keep]) <= 1e-12


def test_nan_workspace_changes_nothing():
    _need_gpu()
    import ctypes as C
    from misonet_amd import _lib
    B, M, T, F, taps, delay = R.SHAPES[0]
    mix, src = (torch.from_numpy(x).cuda() for x in _inputs(B, M, T, F))
    L = _lib.lib()
    o = _lib.WpdOpts(taps, delay, 0.0, 1e-10, 1)
    n = L.misonet_wpd_workspace_bytes(B, F, M, C.byref(o))
    st = _lib.stream_ptr(mix.device)
    got = []
    for fill in (0.0, float("nan")):
        ws = torch.full((n // 8 + 1,), fill, dtype=torch.float64, device="cuda")
        out = torch.full((B, T, F), float("nan"), dtype=torch.complex64, device="cuda")
        w = torch.empty((B, F, M * (taps + 1)), dtype=torch.complex128, device="cuda")
        bad = torch.empty((B, F), dtype=torch.int32, device="cuda")
        _lib.check(L.misonet_wpd(src.data_ptr(), mix.data_ptr(), B, F, M, T, C.byref(o), out.data_ptr(), ws.data_ptr(), n, st))
        _lib.check(L.misonet_wpd_debug(ws.data_ptr(), B, F, M, C.byref(o), w.data_ptr(), bad.data_ptr(), st))
        got.append((out.cpu().numpy(), w.cpu().numpy(), bad.cpu().numpy()))
    assert np.isfinite(got[0][0]).all() and not got[0][2].any()
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert np.array_equal(got[0][2], got[1][2])
    # the library refuses a short workspace and too few frames on the device as it does without one
    assert L.misonet_wpd(src.data_ptr(), mix.data_ptr(), B, F, M, T, C.byref(o), out.data_ptr(), ws.data_ptr(), n - 1, st) == _lib.ENOMEM
    assert L.misonet_wpd(src.data_ptr(), mix.data_ptr(), B, F, M, taps + delay - 1, C.byref(o), out.data_ptr(), ws.data_ptr(), n,
                         st) == _lib.EINVAL


def test_numpy_in_numpy_out():
    _need_gpu()
    from misonet_amd.beamform import Apply_Beamforming
    B, M, T, F, taps, delay = R.SHAPES[1]
    mix, src = _inputs(B, M, T, F)
    out = Apply_Beamforming(src, mix, beamformer="wpd", taps=taps, delay=delay)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.complex64
    assert R.rel(out.numpy(), _ref(R.SHAPES[1], 0, 0.0)[0]) <= R.OUT_BAR
    with pytest.raises(ValueError):
        Apply_Beamforming(src[..., :2], mix[..., :2], beamformer="wpd", taps=taps, delay=delay)      # T <= delay + taps - 1


# ---- the fused pass ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(sd1, sd3):
    """seed weights in the library's default arithmetic"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN")
    m1.cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN")
    m3.cuda(0)
    m3.load_state_dict(sd3)
    return m1.eval(), m3.eval()


def _chunks(B, T):
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    n = 64 * (T - 1)
    wav = np.stack([synthetic_utterance(31 + b, n)[0] for b in range(B)])                    # [B, n, 6]
    return S.stft_hip(torch.from_numpy(wav.astype(np.float32)).cuda()).contiguous()          # [B, 6, T, 129]


def test_fused_pass(nets):
    """step 5 of the fused pass is the drop-in call's kernel through other views: the same bits; a captured graph replays them;
    set_beamformer(None) restores the bits from before; beamform_chunks and beamform_utterance honour the kind"""
    import misonet_amd as mz
    from misonet_amd import _lib
    from misonet_amd.beamform import Apply_Beamforming, Beamformer
    m1, m3 = nets
    B, T = 2, 40
    mix = _chunks(B, T)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    out0, d0 = enh.enhance(mix, want_bf=True)
    spec = dict(kind="wpd", taps=3, delay=2, ref_ch=1)
    enh.set_beamformer(spec)
    assert enh.beamformer == Beamformer(**spec)
    out1, d1 = enh.enhance(mix, want_bf=True, want_miso1=True)
    assert torch.isfinite(torch.view_as_real(d1["bf"])).all() and not torch.equal(d1["bf"], d0["bf"])
    mix_bf = mix.permute(0, 3, 1, 2)                                                         # [B, F, M, T]
    for s in range(2):
        want = Apply_Beamforming(d1["miso1"][:, s].permute(0, 3, 1, 2), mix_bf, beamformer=spec)
        assert torch.equal(torch.view_as_real(d1["bf"][:, s]), torch.view_as_real(want)), s
    # the other entry points that take a Beamformer
    chunks = enh.beamform_chunks(mix)
    assert torch.equal(torch.view_as_real(chunks), torch.view_as_real(d1["bf"]))
    plain = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    assert torch.equal(torch.view_as_real(plain.beamform_chunks(mix, beamformer=spec)), torch.view_as_real(d1["bf"]))
    assert torch.equal(torch.view_as_real(plain.beamform_chunks(mix)), torch.view_as_real(d0["bf"]))
    # a captured graph replays the same bits, and refuses a change of the beamformer while it lives
    cp = enh.capture_graph(mix)
    cp.out.zero_()
    cp.graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(cp.out), torch.view_as_real(out1))
    with pytest.raises(RuntimeError):
        enh.set_beamformer(None)
    del cp
    # bad fields never reach the pipeline; too few frames for the filter are refused by the run
    with pytest.raises(ValueError):
        enh.set_beamformer(dict(kind="wpd", taps=14))
    enh.set_beamformer(dict(kind="wpd", taps=10, delay=40))
    with pytest.raises(_lib.MisonetError):
        enh.enhance(mix)
    # back: the bits from before WPD was set
    enh.set_beamformer(None)
    out2, d2 = enh.enhance(mix, want_bf=True)
    assert torch.equal(torch.view_as_real(out2), torch.view_as_real(out0))
    assert torch.equal(torch.view_as_real(d2["bf"]), torch.view_as_real(d0["bf"]))


def test_beamform_utterance_honours_the_kind(nets):
    """the utterance-wise path: one WPD per speaker over the whole recording's frames = Apply_Beamforming on the same arrays"""
    import misonet_amd as mz
    from misonet_amd import stft as S
    from misonet_amd.beamform import Apply_Beamforming
    m1, m3 = nets
    K, T = 2, 40
    obs = _chunks(K, T)
    clean = obs[:, :2].contiguous()                      # stand-ins for the clean references: they only order the speakers
    enh = mz.Enhancer(m1, None, num_spks=2, ref_ch=0, beamformer=dict(kind="wpd", taps=4, delay=2))
    gap = 100
    got = enh.beamform_utterance(list(obs), list(clean), gap, to_host=False)
    # the same tail by hand
    est = enh.separate(obs, clean)
    e, o = S.istft(est), S.istft(obs)
    n = e.shape[-1]
    keep = [n, n - gap]
    est_t = torch.cat([e[k, ..., :keep[k]] for k in range(K)], dim=-1)
    obs_t = torch.cat([o[k, ..., :keep[k]] for k in range(K)], dim=-1)
    pad = (-obs_t.shape[-1]) % S.HOP
    sig = torch.nn.functional.pad(torch.cat([obs_t[None], est_t], dim=0), (0, pad)).permute(0, 2, 1).contiguous()
    spec = S.stft_hip(sig)
    mix_bf = spec[0].permute(2, 0, 1)[None]
    bf = torch.stack([Apply_Beamforming(spec[1 + s].permute(2, 0, 1)[None], mix_bf, beamformer="wpd", taps=4, delay=2)[0]
                      for s in range(2)])
    assert torch.equal(got, S.istft_int16(bf))
    mvdr = enh.beamform_utterance(list(obs), list(clean), gap, to_host=False, beamformer="mvdr")
    assert mvdr.shape == got.shape and not torch.equal(mvdr, got)
