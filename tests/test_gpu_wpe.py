"""GPU tests of the WPE dereverberation (csrc/wpe.hip, misonet_amd/dereverb.py) against the float64 NumPy restatement of
tests/wpe_ref.py: the output and the filter on every shape that takes another path (order 80, T below one tile, T no multiple
of a tile, batch / bin / microphone edges), the DNN power, bit-reproducibility and independence of the batch, the
pass-through rule, and the recording paths with ``dereverb`` set.

Bars.  Output: rel-L2 <= 2.4e-7 = 4 x 2^-24 (one complex64 rounding of a float64 result is bounded by 2^-24 per element; the
float64 path's own sensitivity on these inputs is three orders below).  Filter G: 100 x the LU-versus-Cholesky difference of
the restatement's G on that case, never below 1e-12 (the margin covers the third summation order the device adds).  The module
prints every figure (``[wpe] ...``).

Measured values (a device run of this module on the MI355X; LAB.md has every line).  Output: 1.8e-8 ... 2.7e-8 on every case, the
one complex64 rounding (the five SHAPES x iterations 1, 3 x diag_load 0, 1e-6; full size 2.529e-8; DNN power 2.446e-8; the bins
beside a zero bin 2.469e-8).  G, as device / LU-versus-Cholesky of the restatement, the worst per shape (always iterations = 3):
(2, 4, 60, 9, 3, 2) 5.6e-14 / 5.9e-14; (1, 2, 40, 5, 2, 1) 1.1e-14 / 1.5e-14; (1, 6, 300, 17, 10, 3) 5.6e-13 / 4.5e-13;
(1, 8, 200, 3, 10, 3) 4.2e-11 / 3.5e-11; (1, 3, 12, 4, 3, 1) 1.9e-12 / 1.1e-12; full size 3.7e-14 / 1.5e-14: within 2.4 x of the
restatement's own difference, against a bar of 100 x.  tests/test_gpu_sg_edges.py holds the same kernel at every order and edge."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import wpe_ref
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

OUT_BAR = 2.4e-7
SHAPES = [(2, 4, 60, 9, 3, 2), (1, 2, 40, 5, 2, 1), (1, 6, 300, 17, 10, 3), (1, 8, 200, 3, 10, 3), (1, 3, 12, 4, 3, 1)]


def _rel(a, b):
    return float(np.linalg.norm((np.asarray(a) - np.asarray(b)).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


@functools.lru_cache(maxsize=None)
def _inputs(B, M, T, F):
    return wpe_ref.reverb_inputs(B, M, T, F)


@functools.lru_cache(maxsize=None)
def _ref(shape, iterations, diag_load):
    """(X, G, fail, LU-versus-Cholesky rel-L2 of G) of the restatement, computed once per case"""
    B, M, T, F, taps, delay = shape
    mix = _inputs(B, M, T, F)
    X, G, bad = wpe_ref.wpe(mix, None, taps, delay, iterations, diag_load)
    _, Gc, _ = wpe_ref.wpe(mix, None, taps, delay, iterations, diag_load, solver="chol")
    return X, G, bad, _rel(Gc, G)


def _run(mix, power=None, **kw):
    from misonet_amd.dereverb import dereverb
    out, dbg = dereverb(torch.from_numpy(mix).cuda(), None if power is None else torch.from_numpy(power).cuda(),
                        return_debug=True, **kw)
    return out.cpu().numpy(), dbg["G"].cpu().numpy(), dbg["fail"].cpu().numpy()


def _check(shape, iterations, diag_load, tag):
    B, M, T, F, taps, delay = shape
    X, G, bad, lu_chol = _ref(shape, iterations, diag_load)
    out, g, fail = _run(_inputs(B, M, T, F), taps=taps, delay=delay, iterations=iterations, diag_load=diag_load)
    e_out, e_g, bar_g = _rel(out, X), _rel(g, G), max(100.0 * lu_chol, 1e-12)
    print(f"[wpe] {tag} {shape} it {iterations} load {diag_load:g}: out {e_out:.3e} (bar {OUT_BAR:g})  G {e_g:.3e} "
          f"(LU vs Cholesky {lu_chol:.3e}, bar {bar_g:.3e})")
    assert out.dtype == np.complex64 and out.shape == X.shape
    assert not bad.any() and not fail.any()
    assert e_out <= OUT_BAR, (tag, e_out)
    assert e_g <= bar_g, (tag, e_g, bar_g)


@pytest.mark.parametrize("diag_load", [0.0, 1e-6])
@pytest.mark.parametrize("iterations", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_restatement(shape, iterations, diag_load):
    _need_gpu()
    _check(shape, iterations, diag_load, "case")


def test_full_size():
    _need_gpu()
    _check((1, 6, 1001, 129, 10, 3), 3, 0.0, "full")


def test_dnn_power():
    """power_dev with iterations = 1 against the restatement with the same power"""
    _need_gpu()
    B, M, T, F, taps, delay = 2, 4, 60, 9, 3, 2
    mix = _inputs(B, M, T, F)
    rng = np.random.default_rng(5)
    power = (np.mean(np.abs(mix) ** 2, axis=1) * rng.uniform(0.5, 2.0, (B, T, F))).astype(np.float32)
    X, G, bad = wpe_ref.wpe(mix, power, taps, delay, 1)
    out, g, fail = _run(mix, power, taps=taps, delay=delay, iterations=1)
    print(f"[wpe] dnn power: out {_rel(out, X):.3e}  G {_rel(g, G):.3e}")
    assert not fail.any() and not bad.any()
    assert _rel(out, X) <= OUT_BAR
    # and it is not the plain first iteration
    assert _rel(out, wpe_ref.wpe(mix, None, taps, delay, 1)[0]) > 1e-4


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    B, M, T, F, taps, delay = 3, 4, 150, 9, 3, 2
    mix = _inputs(B, M, T, F)
    a = _run(mix, taps=taps, delay=delay)
    b = _run(mix, taps=taps, delay=delay)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    one = _run(np.ascontiguousarray(mix[1:2]), taps=taps, delay=delay)
    assert np.array_equal(a[0][1].view(np.uint64), one[0][0].view(np.uint64))
    assert np.array_equal(a[1][1].view(np.uint64), one[1][0].view(np.uint64))


def test_zero_bin_passes_through():
    _need_gpu()
    B, M, T, F, taps, delay = 2, 4, 60, 9, 3, 2
    mix = _inputs(B, M, T, F).copy()
    mix[1, :, :, 4] = 0
    X, G, bad = wpe_ref.wpe(mix, None, taps, delay, 3)
    out, g, fail = _run(mix, taps=taps, delay=delay)
    want = np.zeros((B, F), np.int32)
    want[1, 4] = 1
    assert np.array_equal(fail, want) and np.array_equal(bad, want)
    assert np.array_equal(out[1, :, :, 4].view(np.uint64), mix[1, :, :, 4].view(np.uint64))
    assert not g[1, 4].any()
    keep = np.ones((B, F), bool)
    keep[1, 4] = False
    e = _rel(out.transpose(0, 3, 1, 2)[keep], X.transpose(0, 3, 1, 2)[keep])
    print(f"[wpe] zero bin: the other bins {e:.3e}")
    assert e <= OUT_BAR
    # a non-zero observation with a zero DNN power cannot be factored either: passed through bit for bit
    power = np.ones((B, T, F), np.float32)
    power[0, :, 2] = 0
    out, _, fail = _run(mix, power, taps=taps, delay=delay, iterations=1)
    assert fail[0, 2] == 1 and fail.sum() == 2
    assert np.array_equal(out[0, :, :, 2].view(np.uint64), mix[0, :, :, 2].view(np.uint64))


def test_numpy_in_numpy_out_and_validation():
    _need_gpu()
    from misonet_amd import _lib
    from misonet_amd.dereverb import dereverb
    mix = _inputs(1, 2, 40, 5)
    out = dereverb(mix, taps=2, delay=1)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.complex64
    assert _rel(out.numpy(), wpe_ref.wpe(mix, None, 2, 1, 3)[0]) <= OUT_BAR
    with pytest.raises(ValueError):
        dereverb(mix, taps=41)
    # the library refuses what the Python layer would: in place, and a short workspace
    L = _lib.lib()
    o = _lib.WpeOpts()
    L.misonet_wpe_opts_default(C.byref(o))
    x = torch.from_numpy(_inputs(1, 6, 40, 5)).cuda()
    n = L.misonet_wpe_workspace_bytes(1, 6, 40, 5, C.byref(o))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    st = _lib.stream_ptr(x.device)
    assert L.misonet_wpe(x.data_ptr(), None, 1, 6, 40, 5, C.byref(o), x.data_ptr(), ws.data_ptr(), n, st) == _lib.EINVAL
    assert L.misonet_wpe(x.data_ptr(), None, 1, 6, 40, 5, C.byref(o), y.data_ptr(), ws.data_ptr(), n - 1, st) == _lib.ENOMEM
    assert L.misonet_wpe(x.data_ptr(), None, 1, 6, 1, 5, C.byref(o), y.data_ptr(), ws.data_ptr(), n, st) == _lib.EINVAL


def test_dereverb_wav_is_stft_wpe_istft():
    _need_gpu()
    from misonet_amd import stft as S
    from misonet_amd.dereverb import dereverb, dereverb_wav
    L, M = 12345, 3
    rng = np.random.default_rng(3)
    wav = (0.1 * rng.standard_normal((L, M))).astype(np.float32)
    got = dereverb_wav(wav)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (L, M)
    Lp = -(-L // 64) * 64
    padded = torch.zeros((1, Lp, M), dtype=torch.float32, device="cuda")
    padded[0, :L] = torch.from_numpy(wav).cuda()
    spec = S.stft_hip(padded)
    y = S._istft_hip(dereverb(spec), False)[0, :, :L].T.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    assert 0.0 < np.linalg.norm(got - wav) and np.isfinite(got).all()
    dev = dereverb_wav(torch.from_numpy(wav).cuda(), taps=5)
    assert dev.is_cuda and dev.shape == (L, M)


@pytest.fixture(scope="module")
def nets(sd1, sd3):
    """seed weights in the library's default arithmetic (the dereverberation sits in front of the networks, whatever their mode)"""
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


def _same_score(a, b):
    import json
    return json.dumps(a.as_dict(), sort_keys=True) == json.dumps(b.as_dict(), sort_keys=True)


def test_recording_path(nets):
    """Enhancer(dereverb=...) = dereverb_wav in front of a plain Enhancer, bit for bit; the mixture baseline of the scores stays
    the original observation; set_dereverb(None) restores the plain output"""
    import misonet_amd as mz
    from misonet_amd.dereverb import dereverb_wav
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    chunk = 64 * 40
    L = 2 * chunk - 700
    obs, s0, s1 = synthetic_utterance(21, L)
    plain = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    spec = dict(taps=4, delay=2, iterations=2)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0, dereverb=spec)
    assert enh.dereverb == mz.Dereverb(**spec) and plain.dereverb is None
    base = plain.enhance_recording(obs, [s0, s1], chunk_size=chunk)
    drv = dereverb_wav(obs, **spec)
    want = plain.enhance_recording(drv, [s0, s1], chunk_size=chunk)
    got = enh.enhance_recording(obs, [s0, s1], chunk_size=chunk)
    assert np.array_equal(got, want) and not np.array_equal(got, base)
    # scores: the estimate's figures are those of the dereverberated run, the mixture baseline that of the plain run
    pcm_s, sc = enh.enhance_recording(obs, [s0, s1], chunk_size=chunk, score=True)
    _, sc_plain = plain.enhance_recording(obs, [s0, s1], chunk_size=chunk, score=True)
    _, sc_drv = plain.enhance_recording(drv, [s0, s1], chunk_size=chunk, score=True)
    assert np.array_equal(pcm_s, want)
    assert np.array_equal(sc.si_sdr_mix, sc_plain.si_sdr_mix) and np.array_equal(sc.si_sdr, sc_drv.si_sdr)
    assert np.array_equal(sc.si_sdri, sc.si_sdr - sc_plain.si_sdr_mix)
    res = enh.enhance_recording(obs, [s0, s1], chunk_size=chunk, score=True, bss=True, bss_filt_len=64, stoi=True)
    res_plain = plain.enhance_recording(obs, [s0, s1], chunk_size=chunk, score=True, bss=True, bss_filt_len=64, stoi=True)
    assert np.array_equal(res[2].sdr_mix, res_plain[2].sdr_mix) and np.array_equal(res[3].stoi_mix, res_plain[3].stoi_mix)
    # the coalesced path and the continuous path see the same observation
    many = enh.enhance_recordings([(obs, [s0, s1], "a")], chunk_size=chunk, score=True)
    assert np.array_equal(many["a"][0], want) and _same_score(many["a"][1], sc)
    many = enh.enhance_recordings([(obs, None, "a")], chunk_size=chunk)
    assert np.array_equal(many["a"], enh.enhance_recording(obs, None, chunk_size=chunk))
    cont = enh.enhance_continuous(obs, window=chunk)
    assert np.array_equal(cont, plain.enhance_continuous(drv, window=chunk))
    # back to the plain path
    enh.set_dereverb(None)
    assert enh.dereverb is None
    assert np.array_equal(enh.enhance_recording(obs, [s0, s1], chunk_size=chunk), base)
    with pytest.raises(ValueError):
        enh.set_dereverb(dict(taps=20))          # 6 microphones x 20 taps > 80
