"""GPU tests of the online WPE (csrc/owpe.hip, ``misonet_amd.dereverb.DereverbStream``) against the float64 NumPy restatement of
tests/owpe_ref.py: the output, G, P, fail and n on the smallest shapes at which the kernel takes another path (the smallest of
everything, a stream shorter than the frame ring, orders 63 / 64 / 65 around the wave width, order 80 both ways, a long stream),
each at context 0 and 5 and at alpha 1, 0.999 and 0.98; that the bits do not depend on how the stream is cut into calls; bit
reproducibility and independence of the batch; buffers that held NaN; a planted non-finite sample; an all-zero bin; a captured
graph; and the recording paths with the online form set.

Bars (``owpe_ref``).  Output: rel-L2 <= 2.4e-7 = 4 x 2^-24, one complex64 rounding of a float64 result (the bar of
test_gpu_wpe.py).  G and P: 100 x the rel-L2 by which the restatement's own reversed summation order moves them on that case,
never below 1e-12 (the rule of ``iva_ref.figures``); P exactly Hermitian; fail and n equal.  tests/test_owpe.py shows that each
planted mistake misses these bars.  The module prints every figure (``[owpe] ...``); LAB.md has them.

Measured on an MI355X: the complex64 output equals the restatement's on all 54 cases; G within 2.1e-14 and P within 1.3e-14 rel-L2
(the long stream at alpha 0.98; the restatement's reversed order moves them by 2.3e-14 there), 1e-15 .. 5e-15 at orders 63 .. 80."""
import functools

import numpy as np
import pytest
import torch

import owpe_ref as R
import wpe_ref
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

# (B, M, T, F, taps, delay)
SHAPES = [(2, 2, 40, 5, 3, 1), (1, 1, 1, 1, 1, 1), (1, 3, 4, 3, 10, 3), (1, 7, 60, 2, 9, 2), (1, 8, 60, 2, 8, 2),
          (1, 5, 60, 2, 13, 2), (1, 8, 40, 2, 10, 3), (1, 5, 40, 2, 16, 1), (1, 6, 300, 3, 10, 3)]
IDS = lambda s: "x".join(map(str, s))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(B, M, T, F):
    return wpe_ref.reverb_inputs(B, M, T, F, seed=3)


@functools.lru_cache(maxsize=None)
def _ref(shape, context, alpha):
    """(out, State, bar, own) of the restatement, computed once per case"""
    B, M, T, F, taps, delay = shape
    return R.figures(_inputs(B, M, T, F), taps=taps, delay=delay, context=context, alpha=alpha)


def _run(mix, cuts=None, **kw):
    """the stream on the device, in one call or in the calls ``cuts`` and the rest -> dict(out, G, P, fail, n) as numpy"""
    from misonet_amd.dereverb import DereverbStream
    B, M, T, F = mix.shape
    st = DereverbStream(M, F, B, **kw)
    outs = [st.process(torch.from_numpy(np.ascontiguousarray(mix[:, :, t0:t1])).cuda()) for t0, t1 in R.pieces(T, cuts)]
    d = {k: v.cpu().numpy() for k, v in st._debug().items()}
    d["out"] = torch.cat(outs, dim=2).cpu().numpy()
    return d


def _same(a, b, what=("out", "G", "P", "fail", "n")):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in what)


@pytest.mark.parametrize("alpha", [1.0, 0.999, 0.98])
@pytest.mark.parametrize("context", [0, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_restatement(shape, context, alpha):
    _need_gpu()
    B, M, T, F, taps, delay = shape
    out, st, bar, own = _ref(shape, context, alpha)
    got = _run(_inputs(B, M, T, F), taps=taps, delay=delay, context=context, alpha=alpha)
    e_out, e_g, e_p = R.rel(got["out"], out), R.rel(got["G"], st.G), R.rel(got["P"], st.P)
    print(f"[owpe] case {shape} context {context} alpha {alpha:g}: out {e_out:.3e} (bar {R.OUT_BAR:g})  G {e_g:.3e}  P {e_p:.3e} "
          f"(reversed order {own:.3e}, bar {bar:.3e})")
    assert got["out"].dtype == np.complex64 and got["out"].shape == out.shape
    assert np.array_equal(got["fail"], st.fail) and not st.fail.any() and np.array_equal(got["n"], st.n)
    assert np.array_equal(got["P"], np.conj(np.swapaxes(got["P"], -1, -2))), "P is not exactly Hermitian"
    assert e_out <= R.OUT_BAR, e_out
    assert e_g <= bar and e_p <= bar, (e_g, e_p, bar)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chunk_invariance(shape):
    """the cuts [1, 1, delay, 61, rest]: the bits of the one-call run"""
    _need_gpu()
    B, M, T, F, taps, delay = shape
    kw = dict(taps=taps, delay=delay, context=5, alpha=0.999)
    whole = _run(_inputs(B, M, T, F), **kw)
    cut = _run(_inputs(B, M, T, F), cuts=[1, 1, delay, 61], **kw)
    assert _same(whole, cut)


@pytest.mark.parametrize("shape", [(2, 2, 12, 5, 3, 1), (1, 8, 12, 2, 10, 3)], ids=IDS)
def test_one_frame_per_call(shape):
    _need_gpu()
    B, M, T, F, taps, delay = shape
    kw = dict(taps=taps, delay=delay, context=5, alpha=0.98)
    assert _same(_run(_inputs(B, M, T, F), **kw), _run(_inputs(B, M, T, F), cuts=[1] * T, **kw))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    B, M, T, F, taps, delay = 3, 4, 50, 5, 3, 2
    mix = _inputs(B, M, T, F)
    kw = dict(taps=taps, delay=delay, context=2)
    a, b = _run(mix, **kw), _run(mix, **kw)
    assert _same(a, b)
    one = _run(np.ascontiguousarray(mix[1:2]), **kw)
    assert all(np.array_equal(_bits(one[k][0]), _bits(a[k][1])) for k in ("out", "G", "P", "fail", "n"))


def test_buffers_that_held_nan():
    """reset writes the whole state and the call every output element: NaN in either beforehand changes no bit"""
    _need_gpu()
    from misonet_amd.dereverb import DereverbStream
    B, M, T, F, taps, delay = 2, 3, 20, 4, 3, 2
    mix = _inputs(B, M, T, F)
    kw = dict(taps=taps, delay=delay, context=3)
    want = _run(mix, **kw)
    st = DereverbStream(M, F, B, **kw)
    st.state.fill_(0xFF)
    st.reset()
    x = torch.from_numpy(mix).cuda()
    out = torch.full_like(x, complex(float("nan"), float("nan")))
    st.process_into(x, out)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["out"] = out.cpu().numpy()
    assert _same(want, got)
    assert st.frames_seen == T and not bool(st.fail.any()) and st.filters().shape == (B, F, M * taps, M)


def test_planted_non_finite_sample():
    _need_gpu()
    B, M, T, F, taps, delay = 1, 3, 40, 4, 3, 2
    mix = _inputs(B, M, T, F).copy()
    kw = dict(taps=taps, delay=delay, context=2, alpha=0.99)
    clean = _run(mix, **kw)
    mix[0, 1, 10, 2] = np.nan
    mix[0, 0, 10, 2] = complex(0.0, np.inf)
    got = _run(mix, **kw)
    ref_out, ref = R.owpe(mix, **kw)
    want = np.zeros((B, F), np.int32)
    want[0, 2] = 1
    assert np.array_equal(got["fail"], want) and np.array_equal(ref.fail, want) and (got["n"] == T).all()
    assert np.array_equal(_bits(got["out"][0, :, 10, 2]), _bits(mix[0, :, 10, 2]))               # passed through, bit for bit
    keep = [0, 1, 3]
    for k, ax in (("out", 3), ("G", 1), ("P", 1)):
        assert np.array_equal(_bits(np.take(got[k], keep, axis=ax)), _bits(np.take(clean[k], keep, axis=ax))), k
    assert np.isfinite(got["out"][0, :, 11:, 2]).all() and np.isfinite(got["P"]).all() and np.isfinite(got["G"]).all()
    e = R.rel(np.delete(got["out"], 10, axis=2), np.delete(ref_out, 10, axis=2))
    print(f"[owpe] planted NaN and Inf: the other frames against the restatement {e:.3e}")
    assert e <= R.OUT_BAR


def test_all_zero_bin():
    _need_gpu()
    B, M, T, F, taps, delay = 1, 3, 40, 4, 3, 2
    mix = _inputs(B, M, T, F).copy()
    mix[..., 1] = 0
    got = _run(mix, taps=taps, delay=delay, alpha=0.98)
    assert not got["fail"].any() and np.isfinite(got["out"]).all() and not got["out"][..., 1].any()
    assert np.isfinite(got["P"]).all() and not got["G"][:, 1].any()


def test_captured_graph_replayed_over_three_blocks():
    """one captured misonet_owpe of T = 16, replayed over three successive blocks = the eager stream"""
    _need_gpu()
    from misonet_amd.dereverb import DereverbStream
    B, M, T, F, taps, delay = 1, 4, 48, 5, 4, 2
    mix = _inputs(B, M, T, F)
    kw = dict(taps=taps, delay=delay, context=2)
    want = _run(mix, **kw)
    st = DereverbStream(M, F, B, **kw)
    x = torch.zeros((B, M, 16, F), dtype=torch.complex64, device="cuda")
    y = torch.empty_like(x)
    blocks = [torch.from_numpy(np.ascontiguousarray(mix[:, :, i * 16:(i + 1) * 16])).cuda() for i in range(3)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(stream):
        st.process_into(x, y)                                            # warm-up on the side stream, then a fresh state
        st.reset()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            st.process_into(x, y)
        for blk in blocks:
            x.copy_(blk)
            graph.replay()
            outs.append(y.clone())
        stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["out"] = torch.cat(outs, dim=2).cpu().numpy()
    assert _same(want, got)


def test_numpy_in_numpy_out_and_the_library_refuses():
    _need_gpu()
    import ctypes as C
    from misonet_amd import _lib
    from misonet_amd.dereverb import DereverbStream, dereverb_online
    mix = _inputs(1, 2, 40, 5)
    out = dereverb_online(mix, taps=2, delay=1)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.complex64
    assert R.rel(out.numpy(), R.owpe(mix, 2, 1)[0]) <= R.OUT_BAR
    dev, dbg = dereverb_online(torch.from_numpy(mix).cuda(), taps=2, delay=1, return_debug=True)
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(out.numpy())) and (dbg["n"] == 40).all()
    st = DereverbStream(2, 5, 1, taps=2, delay=1)
    with pytest.raises(ValueError):
        st.process(mix[:, :, :, :4])
    L = _lib.lib()
    x = torch.from_numpy(mix).cuda()
    y = torch.empty_like(x)
    s = _lib.stream_ptr(x.device)
    n = st.state.numel()
    assert L.misonet_owpe(x.data_ptr(), 1, 2, 40, 5, C.byref(st._c), x.data_ptr(), st.state.data_ptr(), n, s) == _lib.EINVAL
    assert L.misonet_owpe(x.data_ptr(), 1, 2, 40, 5, C.byref(st._c), y.data_ptr(), st.state.data_ptr(), n - 1, s) == _lib.ENOMEM
    assert L.misonet_owpe(x.data_ptr(), 1, 2, 0, 5, C.byref(st._c), y.data_ptr(), st.state.data_ptr(), n, s) == _lib.EINVAL
    assert st.frames_seen == 0


def test_dereverb_wav_online_is_stft_owpe_istft():
    _need_gpu()
    from misonet_amd import stft as S
    from misonet_amd.dereverb import OnlineDereverb, dereverb_online, dereverb_wav
    L, M = 12345, 3
    rng = np.random.default_rng(3)
    wav = (0.1 * rng.standard_normal((L, M))).astype(np.float32)
    got = dereverb_wav(wav, online=True)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (L, M)
    Lp = -(-L // 64) * 64
    padded = torch.zeros((1, Lp, M), dtype=torch.float32, device="cuda")
    padded[0, :L] = torch.from_numpy(wav).cuda()
    spec = S.stft_hip(padded)
    y = S._istft_hip(dereverb_online(spec), False)[0, :, :L].T.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(y).view(np.uint32))
    assert 0.0 < np.linalg.norm(got - wav) and np.isfinite(got).all()
    dev = dereverb_wav(torch.from_numpy(wav).cuda(), online=OnlineDereverb(taps=5, alpha=0.99))
    assert dev.is_cuda and dev.shape == (L, M)
    same = dereverb_wav(wav, online=dict(taps=5, alpha=0.99))
    assert np.array_equal(same.view(np.uint32), dev.cpu().numpy().view(np.uint32))
    # online=None is the offline filter, as before
    assert np.array_equal(dereverb_wav(wav, taps=4).view(np.uint32), dereverb_wav(wav, online=None, taps=4).view(np.uint32))
    assert not np.array_equal(dereverb_wav(wav), got)


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


def test_recording_path(nets):
    """Enhancer(dereverb=OnlineDereverb(...)) = dereverb_wav(online=...) in front of a plain Enhancer, bit for bit; with
    dereverb=None the plain output"""
    import misonet_amd as mz
    from misonet_amd.dereverb import dereverb_wav
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    chunk = 64 * 40
    L = 2 * chunk - 700
    obs, s0, s1 = synthetic_utterance(21, L)
    plain = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    spec = mz.OnlineDereverb(taps=4, delay=2, alpha=0.99)
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0, dereverb=spec)
    assert enh.dereverb is spec and plain.dereverb is None
    base = plain.enhance_recording(obs, [s0, s1], chunk_size=chunk)
    drv = dereverb_wav(obs, online=spec)
    want = plain.enhance_recording(drv, [s0, s1], chunk_size=chunk)
    got = enh.enhance_recording(obs, [s0, s1], chunk_size=chunk)
    assert np.array_equal(got, want) and not np.array_equal(got, base)
    cont = enh.enhance_continuous(obs, window=chunk)
    assert np.array_equal(cont, plain.enhance_continuous(drv, window=chunk))
    enh.set_dereverb(None)
    assert enh.dereverb is None
    assert np.array_equal(enh.enhance_recording(obs, [s0, s1], chunk_size=chunk), base)
    enh.set_dereverb(dict(taps=4, delay=2, iterations=2))                 # what Dereverb.of accepts is still the offline filter
    assert enh.dereverb == mz.Dereverb(taps=4, delay=2, iterations=2)
    with pytest.raises(ValueError):
        enh.set_dereverb(mz.OnlineDereverb(taps=20))                      # 6 microphones x 20 taps > 80
