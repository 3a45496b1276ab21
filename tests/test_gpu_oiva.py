"""GPU tests of the online AuxIVA (csrc/oiva.hip, ``misonet_amd.blind.SeparateStream``) against the float64 NumPy restatement of
tests/oiva_ref.py: est, images, W, V, fail and n at every M from 2 to 8, at F = P - 1, P, P + 1 and 2 P + 1 around the bins one
workgroup covers at once (P = ``misonet_oiva_bins_per_pass``), on a single frame of a single bin and on a long stream; that the
bits do not depend on how the stream is cut into calls; bit reproducibility and independence of the batch; buffers that held
NaN; a planted non-finite sample; an all-zero bin; a duplicated microphone; a captured graph; the composition behind the online
WPE; and the recording path with ``online=`` set.

Bars (``oiva_ref``).  est and images: rel-L2 <= 2.4e-7 = 4 x 2^-24, one complex64 rounding of a float64 result.  W and V, against
the clongdouble run of the restatement: 100 x the larger of the rel-L2 distances float64 - clongdouble and float64 - reversed
summation order of the restatement on that case, never below 1e-12 and, for every case here, not above 1e-6 (tests/test_oiva.py
checks that on the CPU).  Every V_k exactly Hermitian; fail and n equal.  The invariants of the definition: sum_k images[k, m] =
x_m within 1e-5 rel-L2, Re(w_k^H V_k w_k) = 1 within 1e-9.  tests/test_oiva.py shows that each planted mistake misses these bars.
The module prints every figure (``[oiva] ...``); LAB.md has them.

Measured on an MI355X: est and images equal the restatement's complex64 on every case (rel-L2 <= 1.4e-15); W within 8.7e-14 and V
within 3.1e-13 rel-L2 of the clongdouble run (M = 6, alpha 0.96; own 3.1e-13 there); |w^H V w - 1| <= 9.3e-14; the sum of the images
within 2.7e-8 of the input."""
import functools

import numpy as np
import pytest
import torch

import iva_ref
import oiva_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))


def shapes(P):
    """(B, M, T, F) of the device cases; P(M) = the bins one workgroup covers at once"""
    p = P(2)
    return [(2, 2, 40, 5), (1, 2, 1, 1), (1, 3, 30, 3), (1, 4, 40, 2), (1, 5, 30, 2), (1, 6, 40, 3), (1, 7, 30, 2), (1, 8, 30, 2),
            (1, 2, 6, p - 1), (1, 2, 6, p), (1, 2, 6, p + 1), (1, 2, 6, 2 * p + 1), (1, 2, 300, 5)]


N_SHAPES = 13
# (model, alpha, images, ref_ch): both models, both alphas, with and without images, one ref_ch != 0
VARIANTS = [("gauss", 0.98, True, 0), ("laplace", 0.96, False, 1), ("gauss", 0.96, False, 0), ("laplace", 0.98, True, 1)]


def _P(M):
    from misonet_amd.blind import bins_per_pass
    return bins_per_pass(M)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(B, M, T, F):
    """M sources at M microphones (the condition of the issue: M <= sources + 1), in the stream layout"""
    return R.to_stream(iva_ref.sparse_mixture(B, M, M, T, F, seed=B + M + T + F)[0])


@functools.lru_cache(maxsize=None)
def _ref(shape, model, alpha, ref_ch):
    return R.figures(_inputs(*shape), model=model, alpha=alpha, ref_ch=ref_ch)


def _run(mix, cuts=None, images=True, **kw):
    """the stream on the device, in one call or in the calls ``cuts`` and the rest -> dict(est, images, W, V, fail, n) as numpy"""
    from misonet_amd.blind import SeparateStream
    B, M, T, F = mix.shape
    st = SeparateStream(M, F, B, **kw)
    ests, imgs = [], []
    for t0, t1 in R.pieces(T, cuts):
        out = st.process(torch.from_numpy(np.ascontiguousarray(mix[:, :, t0:t1])).cuda(), images=images)
        ests.append(out[0] if images else out)
        if images:
            imgs.append(out[1])
    d = {k: v.cpu().numpy() for k, v in st._debug().items()}
    d["est"] = torch.cat(ests, dim=2).cpu().numpy()
    if images:
        d["images"] = torch.cat(imgs, dim=3).cpu().numpy()
    return d


ALL = ("est", "images", "W", "V", "fail", "n")


def _same(a, b, what=ALL):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in what)


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: f"{v[0]}-{v[1]}-{'img' if v[2] else 'est'}-ref{v[3]}")
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_against_restatement(i, variant):
    _need_gpu()
    shape = shapes(_P)[i]
    model, alpha, images, ref_ch = variant
    ref = _ref(shape, model, alpha, ref_ch)
    st, ext, bar = ref["st"], ref["ext"], ref["bar"]
    got = _run(_inputs(*shape), images=images, model=model, alpha=alpha, ref_ch=ref_ch)
    e_est = R.rel(got["est"], ref["est"])
    e_img = R.rel(got["images"], ref["images"]) if images else 0.0
    e_w, e_v = R.rel(got["W"], ext.W), R.rel(got["V"], ext.V)
    unit = R.unit_norm_error(got["W"], got["V"])
    e_sum = R.image_sum_error(got["images"], _inputs(*shape), got["fail"]) if images else 0.0
    print(f"[oiva] case {shape} {model} alpha {alpha:g} ref {ref_ch}: est {e_est:.3e} images {e_img:.3e} (bar {R.OUT_BAR:g})  "
          f"W {e_w:.3e}  V {e_v:.3e} (own {ref['own']:.3e}, bar {bar:.3e})  |w^H V w - 1| {unit:.3e}  sum of images {e_sum:.3e}")
    assert bar <= R.BAR_CAP
    assert got["est"].dtype == np.complex64 and got["est"].shape == ref["est"].shape
    assert np.array_equal(got["fail"], st.fail) and not st.fail.any() and np.array_equal(got["n"], st.n)
    assert R.hermitian(got["V"]), "V is not exactly Hermitian"
    assert e_est <= R.OUT_BAR and e_img <= R.OUT_BAR, (e_est, e_img)
    assert e_w <= bar and e_v <= bar, (e_w, e_v, bar)
    assert unit <= 1e-9 and e_sum <= 1e-5, (unit, e_sum)


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_cut_invariance(i):
    """the cuts [1, 1, 2, 17, rest]: the bits of the one-call run"""
    _need_gpu()
    shape = shapes(_P)[i]
    whole = _run(_inputs(*shape), alpha=0.96)
    cut = _run(_inputs(*shape), cuts=[1, 1, 2, 17], alpha=0.96)
    assert _same(whole, cut)


@pytest.mark.parametrize("shape", [(2, 2, 12, 5), (1, 8, 12, 2)], ids=IDS)
def test_one_frame_per_call(shape):
    _need_gpu()
    T = shape[2]
    assert _same(_run(_inputs(*shape), model="laplace"), _run(_inputs(*shape), cuts=[1] * T, model="laplace"))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    mix = _inputs(3, 4, 50, 5)
    a, b = _run(mix), _run(mix)
    assert _same(a, b)
    one = _run(np.ascontiguousarray(mix[1:2]))
    assert all(np.array_equal(_bits(one[k][0]), _bits(a[k][1])) for k in ALL)


def test_buffers_that_held_nan():
    """reset writes the whole state and the call every output element: NaN in either beforehand changes no bit"""
    _need_gpu()
    from misonet_amd.blind import SeparateStream
    B, M, T, F = 2, 3, 20, 4
    mix = _inputs(B, M, T, F)
    want = _run(mix)
    st = SeparateStream(M, F, B)
    st.state.fill_(0xFF)
    st.reset()
    x = torch.from_numpy(mix).cuda()
    nan = complex(float("nan"), float("nan"))
    est = torch.full_like(x, nan)
    img = torch.full((B, M, M, T, F), nan, dtype=torch.complex64, device="cuda")
    st.process_into(x, est, img)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["est"], got["images"] = est.cpu().numpy(), img.cpu().numpy()
    assert _same(want, got)
    assert st.frames_seen == T and not bool(st.fail.any())
    assert st.demixing().shape == (B, F, M, M) and st.covariance().shape == (B, F, M, M, M)


def test_planted_non_finite_sample():
    _need_gpu()
    B, M, T, F = 1, 3, 40, 4
    mix = _inputs(B, M, T, F).copy()
    mix[0, 1, 10, 2] = complex(np.nan, 0.0)
    before = _run(mix[:, :, :10])
    at = _run(mix[:, :, :11])
    got = _run(mix)
    est, img, ref = R.oiva(mix)
    want = np.zeros((B, F), np.int32)
    want[0, 2] = 1
    assert np.array_equal(got["fail"], want) and np.array_equal(ref.fail, want) and (got["n"] == T).all()
    assert not got["est"][0, :, 10, 2].any() and not got["images"][0, :, :, 10, 2].any()
    for k in ("W", "V"):                                             # that bin's state is unchanged by the frame
        assert np.array_equal(_bits(at[k][0, 2]), _bits(before[k][0, 2])), k
        assert not np.array_equal(_bits(at[k][0, 1]), _bits(before[k][0, 1])), k
    e_est, e_img = R.rel(got["est"], est), R.rel(got["images"], img)
    _, _, ext = R.oiva(mix, dtype=np.clongdouble)
    _, _, rev = R.oiva(mix, reverse=True)
    own = max(R.rel(ref.W, ext.W), R.rel(ref.V, ext.V), R.rel(ref.W, rev.W), R.rel(ref.V, rev.V))
    bar = max(100.0 * own, R.STATE_FLOOR)
    e_w, e_v = R.rel(got["W"], ext.W), R.rel(got["V"], ext.V)
    print(f"[oiva] planted NaN: est {e_est:.3e} images {e_img:.3e}  W {e_w:.3e}  V {e_v:.3e} (bar {bar:.3e})")
    assert e_est <= R.OUT_BAR and e_img <= R.OUT_BAR and e_w <= bar and e_v <= bar and bar <= R.BAR_CAP
    assert np.isfinite(got["est"]).all() and np.isfinite(got["W"]).all() and np.isfinite(got["V"]).all()


def test_all_zero_bin():
    _need_gpu()
    mix = _inputs(1, 3, 40, 4).copy()
    mix[..., 1] = 0
    got = _run(mix)
    assert np.isfinite(got["est"]).all() and np.isfinite(got["images"]).all()
    assert not got["est"][..., 1].any() and np.isfinite(got["W"]).all() and np.isfinite(got["V"]).all()
    assert not (got["fail"] & 1).any()


def test_duplicated_microphone():
    """Two identical microphones and a V_0 far below the data (init 1e-300): alpha V + (1 - alpha) phi x x^H rounds to the exactly
    singular rank-one matrix a [[1, 1], [1, 1]], with W = I the elimination of W V_k meets the pivot a - a = 0, and every row
    update is dropped: the solve fails, fail bit 1 is set, nothing is NaN and the state stays finite"""
    _need_gpu()
    mix = _inputs(1, 2, 20, 3).copy()
    mix[:, 1] = mix[:, 0]
    got = _run(mix, init=1e-300)
    est, img, ref = R.oiva(mix, init=1e-300)
    print(f"[oiva] duplicated microphone: fail {sorted(set(got['fail'].ravel().tolist()))} (restatement "
          f"{sorted(set(ref.fail.ravel().tolist()))})")
    assert (got["fail"] & 6).all() and not (got["fail"] & 1).any() and np.array_equal(got["fail"], ref.fail)
    for k in ("est", "images", "W", "V"):
        assert np.isfinite(got[k]).all(), k
    assert R.hermitian(got["V"])


def test_captured_graph_replayed_twice():
    """one captured misonet_oiva of T = 16, replayed over two successive blocks = two eager calls, bit for bit (a single stream
    of launches: no parallel branches in the graph)"""
    _need_gpu()
    from misonet_amd.blind import SeparateStream
    B, M, T, F = 1, 4, 32, 5
    mix = _inputs(B, M, T, F)
    want = _run(mix, cuts=[16])
    st = SeparateStream(M, F, B)
    x = torch.zeros((B, M, 16, F), dtype=torch.complex64, device="cuda")
    est = torch.empty_like(x)
    img = torch.empty((B, M, M, 16, F), dtype=torch.complex64, device="cuda")
    blocks = [torch.from_numpy(np.ascontiguousarray(mix[:, :, i * 16:(i + 1) * 16])).cuda() for i in range(2)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    ests, imgs = [], []
    with torch.cuda.stream(stream):
        st.process_into(x, est, img)                                     # warm-up on the side stream, then a fresh state
        st.reset()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            st.process_into(x, est, img)
        for blk in blocks:
            x.copy_(blk)
            graph.replay()
            ests.append(est.clone())
            imgs.append(img.clone())
        stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["est"], got["images"] = torch.cat(ests, dim=2).cpu().numpy(), torch.cat(imgs, dim=3).cpu().numpy()
    assert _same(want, got)


def test_composition_behind_online_wpe():
    """DereverbStream.process -> SeparateStream.process in blocks of 16 frames = the same composition in one call"""
    _need_gpu()
    from misonet_amd.blind import SeparateStream
    from misonet_amd.dereverb import DereverbStream
    B, M, T, F = 1, 3, 50, 5
    x = torch.from_numpy(_inputs(B, M, T, F)).cuda()

    def run(step):
        d, s = DereverbStream(M, F, B, taps=3, delay=2), SeparateStream(M, F, B)
        outs = [s.process(d.process(x[:, :, t:t + step].contiguous()), images=True) for t in range(0, T, step)]
        dbg = {k: v.cpu().numpy() for k, v in s._debug().items()}
        dbg["est"] = torch.cat([o[0] for o in outs], dim=2).cpu().numpy()
        dbg["images"] = torch.cat([o[1] for o in outs], dim=3).cpu().numpy()
        return dbg
    whole, blocks = run(T), run(16)
    assert _same(whole, blocks) and np.isfinite(whole["est"]).all() and whole["est"].any()


def test_numpy_in_numpy_out_and_the_library_refuses():
    _need_gpu()
    import ctypes as C
    from misonet_amd import _lib
    from misonet_amd.blind import SeparateStream, auxiva_online
    mix = _inputs(1, 2, 40, 5)
    est, img = auxiva_online(mix, images=True)
    assert isinstance(est, torch.Tensor) and est.device.type == "cpu" and est.dtype == torch.complex64
    assert img.shape == (1, 2, 2, 40, 5)
    assert R.rel(est.numpy(), R.oiva(mix)[0]) <= R.OUT_BAR
    dev, dbg = auxiva_online(torch.from_numpy(mix).cuda(), return_debug=True)
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(est.numpy())) and (dbg["n"] == 40).all()
    st = SeparateStream(2, 5, 1)
    with pytest.raises(ValueError):
        st.process(mix[:, :, :, :4])
    L = _lib.lib()
    x = torch.from_numpy(mix).cuda()
    y = torch.empty_like(x)
    s = _lib.stream_ptr(x.device)
    n = st.state.numel()
    assert L.misonet_oiva(x.data_ptr(), 1, 2, 40, 5, C.byref(st._c), x.data_ptr(), None, st.state.data_ptr(), n, s) == _lib.EINVAL
    assert L.misonet_oiva(x.data_ptr(), 1, 2, 40, 5, C.byref(st._c), y.data_ptr(), None, st.state.data_ptr(), n - 1, s) == _lib.ENOMEM
    assert L.misonet_oiva(x.data_ptr(), 1, 2, 0, 5, C.byref(st._c), y.data_ptr(), None, st.state.data_ptr(), n, s) == _lib.EINVAL
    assert st.frames_seen == 0


def test_recording_path():
    """separate_recording(online=True) on 1 s of the real recording: int16 [2, L], the same bytes twice; online=None is the call
    without the argument; beamform=True with online raises"""
    _need_gpu()
    from misonet_amd.blind import BlindSeparator
    wav, _, fs = iva_ref.g8_sample()
    wav = np.ascontiguousarray(wav[:fs])
    sep = BlindSeparator(num_spks=2, num_ch=2)
    a = sep.separate_recording(wav, online=True)
    b = sep.separate_recording(wav, beamform=False, online=True)
    assert a.dtype == np.int16 and a.shape == (2, fs) and a.any() and a.tobytes() == b.tobytes()
    d = sep.separate_recording(wav, online=dict(alpha=0.96), dereverb=dict(taps=3))
    assert d.shape == (2, fs) and d.tobytes() != a.tobytes()
    assert sep.separate_recording(wav, online=None).tobytes() == sep.separate_recording(wav).tobytes()
    with pytest.raises(ValueError):
        sep.separate_recording(wav, beamform=True, online=True)
    with pytest.raises(ValueError):
        sep.separate_recording(wav, dereverb=True)                        # the online WPE belongs to the online path
