"""GPU tests of the blind separation (csrc/iva.hip, ``misonet_amd.blind``) against the float64 NumPy restatement of
tests/iva_ref.py: images, Y, A, the eigenvectors, power, the chosen rows and the failure flags on every shape that takes
another path (T = 1, the wave and workgroup edges of the strided partials, odd M, the largest K and M, the last resident and the
first streamed frame count for K = 2 and K = 8), both models, 0, 1 and 20 iterations; bit-reproducibility and independence of
the batch; buffers full of NaN; a NaN planted in one bin; an all-zero bin and an all-zero tail; a captured HIP graph; and
``BlindSeparator`` against the drop-in composition and, on the real six-microphone mixture of tests/golden, against the
restatement's SI-SDR improvement.

Bars (tests/iva_ref.py ``figures``).  Images: rel-L2 <= 2.4e-7, one complex64 rounding.  Y, A, eigenvectors, power: rel-L2
<= 100 x the restatement's permuted-order difference on that case, never below 1e-12.  The module prints every figure
(``[iva] ...``); LAB.md has them."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import iva_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
IDS = lambda s: "x".join(map(str, s))


def _resident(K):
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return int(_lib.lib().misonet_auxiva_resident_frames(K))


SHAPES = R.shapes(_resident)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.case_inputs(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, model, iterations):
    """(the restatement, the restatement with every sum over t in a permuted order), computed once per case"""
    B, S, K, M, T, F = shape
    mix, ref_ch = _inputs(shape), R.case_ref_ch(shape)
    order = np.random.default_rng(5).permutation(T)
    return (R.auxiva(mix, S, K, iterations, model, ref_ch=ref_ch),
            R.auxiva(mix, S, K, iterations, model, ref_ch=ref_ch, frame_order=order))


def _run(mix, S, **kw):
    from misonet_amd.blind import auxiva
    images, order, dbg = auxiva(torch.from_numpy(np.ascontiguousarray(mix)).cuda(), S, return_order=True, return_debug=True, **kw)
    out = dict(images=images.cpu().numpy(), order=order.cpu().numpy())
    out.update({k: v.cpu().numpy() for k, v in dbg.items()})
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[x.dtype.itemsize])


NAMES = ("images", "order", "Y", "A", "evec", "power", "fail")


def _same(a, b, names=NAMES):
    return all(np.array_equal(_bits(a[n]), _bits(b[n])) for n in names)


@pytest.mark.parametrize("iterations", [0, 1, 20])
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_restatement(shape, model, iterations):
    """Every figure against its bar, the chosen rows and the flags.  The case 1x2x2x3x1x4 (T = 1) is a bin of rank one with
    K = 2: its second eigenvector, its second row of Y and that row's images are 0 by the rank rule of the PCA."""
    _need_gpu()
    B, S, K, M, T, F = shape
    mix = _inputs(shape)
    want, perm = _ref(shape, model, iterations)
    got = _run(mix, S, iterations=iterations, model=model, channels=K, ref_ch=R.case_ref_ch(shape))
    fig = R.figures(got, want, perm)
    print(f"[iva] {shape} {model} {iterations} it: " + "  ".join(f"{k} {v:.3e} (bar {b:.3e})" for k, (v, b) in fig.items()))
    assert got["images"].dtype == np.complex64 and got["images"].shape == want["images"].shape == (B, S, F, M, T)
    assert got["Y"].shape == (B, F, K, T) and got["A"].shape == got["evec"].shape == (B, F, M, K)
    assert not want["fail"].any() and not got["fail"].any()
    assert np.array_equal(got["order"], want["order"]), (got["order"], want["order"], want["power"])
    assert not R.missed(fig), fig


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    mix = R.sparse_mixture(3, 3, 4, 150, 9, seed=3)[0]
    kw = dict(iterations=5, channels=3, ref_ch=1)
    a, b = _run(mix, 2, **kw), _run(mix, 2, **kw)
    assert _same(a, b) and not a["fail"].any() and np.isfinite(a["images"]).all()
    for i in range(3):
        one = _run(mix[i:i + 1], 2, **kw)
        for n in NAMES:
            assert np.array_equal(_bits(a[n][i]), _bits(one[n][0])), (i, n)


def _raw(y, S, K, opts, fill):
    """misonet_auxiva on buffers that held ``fill``; everything it exports, as numpy"""
    from misonet_amd import _lib
    L = _lib.lib()
    B, F, M, T = y.shape
    n = L.misonet_auxiva_workspace_bytes(B, S, K, F, M, T)
    st = _lib.stream_ptr(y.device)
    ws = torch.full((n // 8 + 1,), fill, dtype=torch.float64, device="cuda")
    images = torch.full((B, S, F, M, T), fill, dtype=torch.complex64, device="cuda")
    order = torch.full((B, S), -7, dtype=torch.int32, device="cuda")
    dbg = dict(Y=torch.empty((B, F, K, T), dtype=torch.complex128, device="cuda"),
               A=torch.empty((B, F, M, K), dtype=torch.complex128, device="cuda"),
               evec=torch.empty((B, F, M, K), dtype=torch.complex128, device="cuda"),
               power=torch.empty((B, K), dtype=torch.float64, device="cuda"),
               fail=torch.empty((B, F), dtype=torch.int32, device="cuda"))
    _lib.check(L.misonet_auxiva(y.data_ptr(), B, S, F, M, T, C.byref(opts), images.data_ptr(), order.data_ptr(), ws.data_ptr(),
                                n, st))
    _lib.check(L.misonet_auxiva_debug(ws.data_ptr(), B, K, F, M, T, dbg["Y"].data_ptr(), dbg["A"].data_ptr(),
                                      dbg["evec"].data_ptr(), dbg["power"].data_ptr(), dbg["fail"].data_ptr(), st))
    r = dict(images=images.cpu().numpy(), order=order.cpu().numpy())
    r.update({k: v.cpu().numpy() for k, v in dbg.items()})
    return r, (ws, images, n)


@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[9]], ids=IDS)
def test_nan_buffers_change_nothing(shape):
    """a workspace and output buffers that held NaN before the call: the same bits as with zeros, on the resident and on the
    streaming path; and the argument checks of the library on the device as without one"""
    _need_gpu()
    from misonet_amd import _lib
    B, S, K, M, T, F = shape
    y = torch.from_numpy(_inputs(shape)).cuda()
    o = _lib.IvaOpts(3, 0, K, R.case_ref_ch(shape), 1e-10)
    (r0, _), (r1, (ws, images, n)) = _raw(y, S, K, o, 0.0), _raw(y, S, K, o, float("nan"))
    assert np.isfinite(r0["images"]).all() and np.isfinite(r0["Y"]).all() and not r0["fail"].any()
    assert _same(r0, r1)
    L = _lib.lib()
    st = _lib.stream_ptr(y.device)
    assert L.misonet_auxiva(y.data_ptr(), B, S, F, M, T, C.byref(o), images.data_ptr(), None, ws.data_ptr(), n - 1, st) == _lib.ENOMEM
    bad = _lib.IvaOpts(3, 2, K, 0, 1e-10)
    assert L.misonet_auxiva(y.data_ptr(), B, S, F, M, T, C.byref(bad), images.data_ptr(), None, ws.data_ptr(), n, st) == _lib.EINVAL


def test_nan_in_one_bin():
    """fail = 1 there and zero images; every other bin carries the bits of the run with that bin zeroed"""
    _need_gpu()
    shape = SHAPES[0]
    B, S, K, M, T, F = shape
    mix = _inputs(shape).copy()
    kw = dict(iterations=20, channels=K, ref_ch=R.case_ref_ch(shape))
    zeroed = mix.copy()
    zeroed[1, 4] = 0
    mix[1, 4, 2, 17] = complex(np.nan, 0.0)
    mix[1, 4, 0, 3] = complex(0.0, np.inf)
    got, base = _run(mix, S, **kw), _run(zeroed, S, **kw)
    flags = np.zeros((B, F), np.int32)
    flags[1, 4] = 1
    assert np.array_equal(got["fail"], flags) and not base["fail"].any()
    assert np.array_equal(R.auxiva(mix, S, K, ref_ch=kw["ref_ch"])["fail"], flags)
    assert not got["images"][1, :, 4].any() and not got["Y"][1, 4].any() and not got["A"][1, 4].any()
    assert np.isfinite(got["images"]).all() and np.isfinite(got["power"]).all()
    keep = flags == 0
    for n in ("Y", "A", "evec"):
        assert np.array_equal(_bits(got[n][keep]), _bits(base[n][keep])), n
    assert np.array_equal(_bits(got["images"].transpose(0, 2, 1, 3, 4)[keep]), _bits(base["images"].transpose(0, 2, 1, 3, 4)[keep]))
    assert np.array_equal(_bits(got["power"]), _bits(base["power"])) and np.array_equal(got["order"], base["order"])


def test_zero_bin_and_zero_tail():
    """an all-zero bin and an all-zero tail of frames (the padding of a last chunk): finite output, zero images in the bin and
    in the tail, no flag; and the figures of the restatement hold"""
    _need_gpu()
    shape = SHAPES[0]
    B, S, K, M, T, F = shape
    mix = _inputs(shape).copy()
    mix[0, 2] = 0
    mix[..., T - 7:] = 0
    ref_ch = R.case_ref_ch(shape)
    got = _run(mix, S, iterations=20, channels=K, ref_ch=ref_ch)
    assert not got["fail"].any() and all(np.isfinite(got[n]).all() for n in ("images", "Y", "A", "evec", "power"))
    assert not got["images"][0, :, 2].any() and not got["images"][..., T - 7:].any()
    want = R.auxiva(mix, S, K, ref_ch=ref_ch)
    perm = R.auxiva(mix, S, K, ref_ch=ref_ch, frame_order=np.random.default_rng(5).permutation(T))
    keep = np.ones((B, F), bool)
    keep[0, 2] = False                                  # the eigenvectors of a zero matrix are anybody's: not compared
    cut = lambda r: dict(r, evec=r["evec"][keep])
    fig = R.figures(cut(got), cut(want), cut(perm))
    print(f"[iva] zero bin and tail {shape}: " + "  ".join(f"{k} {v:.3e} (bar {b:.3e})" for k, (v, b) in fig.items()))
    assert not R.missed(fig), fig
    assert np.array_equal(got["order"], want["order"])


def test_hip_graph():
    """misonet_auxiva captured once, replayed twice with new inputs copied in: the bits of the eager call"""
    _need_gpu()
    from misonet_amd import _lib
    shape = SHAPES[0]
    B, S, K, M, T, F = shape
    L = _lib.lib()
    o = _lib.IvaOpts(20, 0, K, R.case_ref_ch(shape), 1e-10)
    inputs = [torch.from_numpy(R.sparse_mixture(B, K, M, T, F, seed=50 + i)[0]).cuda() for i in range(3)]
    eager = [_raw(y, S, K, o, 0.0)[0] for y in inputs]
    assert not np.array_equal(eager[1]["images"], eager[2]["images"])
    n = L.misonet_auxiva_workspace_bytes(B, S, K, F, M, T)
    y = inputs[0].clone()
    ws = torch.zeros((n // 8 + 1,), dtype=torch.float64, device="cuda")
    images = torch.zeros((B, S, F, M, T), dtype=torch.complex64, device="cuda")
    order = torch.zeros((B, S), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _lib.check(L.misonet_auxiva(y.data_ptr(), B, S, F, M, T, C.byref(o), images.data_ptr(), order.data_ptr(),
                                        ws.data_ptr(), n, _lib.stream_ptr(y.device)))
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        y.copy_(inputs[i])
        images.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(images.cpu().numpy()), _bits(eager[i]["images"])), i
        assert np.array_equal(order.cpu().numpy(), eager[i]["order"]), i


def test_numpy_in_numpy_out():
    _need_gpu()
    from misonet_amd.blind import auxiva
    shape = SHAPES[1]
    B, S, K, M, T, F = shape
    mix = _inputs(shape)
    images, order = auxiva(mix, S, return_order=True)
    assert isinstance(images, torch.Tensor) and images.device.type == "cpu" and images.dtype == torch.complex64
    assert order.device.type == "cpu" and order.dtype == torch.int32 and tuple(order.shape) == (B, S)
    assert R.rel(images.numpy(), _ref(shape, "gauss", 20)[0]["images"]) <= R.OUT_BAR
    only = auxiva(torch.from_numpy(mix).cuda(), S, blind=dict(iterations=20))
    assert only.is_cuda and torch.equal(torch.view_as_real(only.cpu()), torch.view_as_real(images))


# ---- BlindSeparator ---------------------------------------------------------------------------------------------------------
def _chunks(B, T):
    from misonet_amd import stft as S
    from misonet_amd.weights import synthetic_utterance
    n = 64 * (T - 1)
    wav = np.stack([synthetic_utterance(31 + b, n)[0] for b in range(B)])                    # [B, n, 6]
    return S.stft_hip(torch.from_numpy(wav.astype(np.float32)).cuda()).contiguous()          # [B, 6, T, 129]


def _eq(a, b):
    return a.shape == b.shape and torch.equal(torch.view_as_real(a.contiguous()), torch.view_as_real(b.contiguous()))


def test_blind_separator_is_the_drop_in_composition():
    """separate = auxiva in the layout of Enhancer.separate; beamform_chunks = the drop-in entry points one after the other,
    bit for bit, with a per-speaker beamformer, a joint one and the guided clustering in between"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd.beamform import Apply_Beamforming, Apply_Beamforming_Joint, JointBeamformer
    from misonet_amd.refine import refined_images
    mix = _chunks(2, 40)
    mix_bf = mix.permute(0, 3, 1, 2).contiguous()
    images = mz.auxiva(mix_bf, 2, iterations=10, ref_ch=1)
    assert torch.isfinite(torch.view_as_real(images)).all()
    blind = dict(iterations=10)
    sep = mz.BlindSeparator(2, 6, ref_ch=1, blind=blind)
    est = sep.separate(mix)
    assert tuple(est.shape) == (2, 2, 6, 40, 129) and _eq(est, images.permute(0, 1, 3, 4, 2))
    sep = mz.BlindSeparator(2, 6, ref_ch=1, blind=blind, beamformer="souden")
    want = torch.stack([Apply_Beamforming(images[:, s], mix_bf, beamformer="souden") for s in range(2)], dim=1)
    got = sep.beamform_chunks(mix)
    assert tuple(got.shape) == (2, 2, 40, 129) and _eq(got, want)
    jb = JointBeamformer("lcmv")
    sep = mz.BlindSeparator(2, 6, ref_ch=1, blind=blind, beamformer=jb)
    assert _eq(sep.beamform_chunks(mix), Apply_Beamforming_Joint(images, mix_bf, jb))
    sep = mz.BlindSeparator(2, 6, ref_ch=1, blind=blind, refine="guided")
    refined = refined_images(images, mix_bf, "guided")
    want = torch.stack([Apply_Beamforming(refined[:, s], mix_bf) for s in range(2)], dim=1)
    got = sep.beamform_chunks(mix)
    assert _eq(got, want) and not _eq(got, torch.stack([Apply_Beamforming(images[:, s], mix_bf) for s in range(2)], dim=1))
    with pytest.raises(ValueError):
        sep.separate(mix[:, :5])
    with pytest.raises(ValueError):
        mz.BlindSeparator(2, 6, blind=dict(channels=7))


def test_separate_recording_on_real_speech(tmp_path):
    """the real six-microphone two-speaker mixture: int16 [2, 32000]; with ``beamform=False`` the SI-SDR improvement through
    misonet_amd.score within 0.1 dB of the restatement's for the same options; the files are the returned array"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import score as SC, stft as S
    wav, clean, fs = R.g8_sample()
    sep = mz.BlindSeparator(2, 6, ref_ch=0)
    path = str(tmp_path / "out" / "g8")
    pcm = sep.separate_recording(wav, save_path=path, fs=fs, beamform=False)
    assert isinstance(pcm, np.ndarray) and pcm.dtype == np.int16 and pcm.shape == (2, 32000)
    sc = SC.score_waves(pcm, clean, wav[:, 0], fs=fs)
    got = float(np.mean(sc.si_sdr_best - sc.si_sdr_mix))
    r = R.auxiva_item(R.stft(wav), 2)
    est = np.stack([R.istft(r["images"][s, :, 0, :], wav.shape[0]) for s in range(2)])
    _, want = R.si_sdr_improvement(est, clean.astype(np.float64), wav[:, 0].astype(np.float64))
    print(f"[iva] g8 sample, defaults, image at microphone 0: SI-SDR improvement {got:.2f} dB (restatement {want:.2f} dB)")
    assert abs(got - want) <= 0.1, (got, want)
    for s in range(2):
        S.write_wav_pcm24(str(tmp_path / f"again_{s}.wav"), pcm[s], fs)
        assert open(f"{path}_{s}.wav", "rb").read() == open(tmp_path / f"again_{s}.wav", "rb").read()
    bf = sep.separate_recording(wav, fs=fs)                                    # the MVDR on the images
    assert bf.dtype == np.int16 and bf.shape == (2, 32000) and not np.array_equal(bf, pcm)
    sb = SC.score_waves(bf, clean, wav[:, 0], fs=fs)
    print(f"[iva] g8 sample, defaults, then MVDR: SI-SDR improvement {float(np.mean(sb.si_sdr_best - sb.si_sdr_mix)):.2f} dB")
    pcm2, srmr = sep.separate_recording(wav, fs=fs, beamform=False, srmr=True)
    assert np.array_equal(pcm2, pcm) and isinstance(srmr, SC.Srmr)
