"""GPU tests of the online beamformer (csrc/obf.hip, ``misonet_amd.beamform.BeamformStream``) against the float64 NumPy restatement
of tests/obf_ref.py: out, Phi_s, Phi_n, w, fail and n at every M from 2 to 8, with S < M, S = M and S = 1, at F = C - 1, C, C + 1
around the cells one workgroup covers (C = ``misonet_obf_cells_per_block``), on a single frame of a single bin and on long
streams; that the bits do not depend on how the stream is cut into calls; bit reproducibility and independence of the batch;
buffers that held NaN; planted non-finite samples; a source that starts silent; the pivot failure; the distortionless identity; a
captured graph; the composition behind the online WPE and the online AuxIVA; and the recording path with
``beamform=OnlineBeamformer()``.

Bars (``obf_ref``).  out: rel-L2 <= 2.4e-7 = 4 x 2^-24, one complex64 rounding of a float64 result.  Phi_s, Phi_n and w, against
the clongdouble run of the restatement: 100 x the larger of the rel-L2 distances float64 - clongdouble and float64 - reversed
summation order of the restatement on that case, never below 1e-12 and, for every case here, not above 1e-6 (tests/test_obf.py
checks that on the CPU).  Phi_s and Phi_n exactly Hermitian; fail and n equal.  tests/test_obf.py shows that each planted mistake
misses these bars.  The module prints every figure (``[obf] ...``); LAB.md has them.

Measured on an MI355X: out equals the restatement's complex64 on every case (rel-L2 0); Phi_s within 3.5e-16, Phi_n within 4.3e-16
and w within 4.2e-14 rel-L2 of the clongdouble run (M = 6, T = 300, noise "mix"; own 4.7e-14 there); w^H a = a[ref] within 4.5e-16
on the rank-one source."""
import functools

import numpy as np
import pytest
import torch

import iva_ref
import obf_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

IDS = lambda s: "x".join(map(str, s))
CUTS = [1, 1, 2, 17]


def shapes(C):
    """(B, S, M, T, F) of the device cases; C(M) = the cells one workgroup covers"""
    c2, c6 = C(2), C(6)
    return [(2, 2, 2, 40, 5), (1, 1, 2, 1, 1), (1, 3, 3, 30, 3), (1, 2, 4, 40, 2), (1, 5, 5, 30, 2), (1, 6, 6, 40, 3), (1, 7, 7, 30, 2),
            (1, 8, 8, 30, 2), (1, 1, 2, 6, c2 - 1), (1, 1, 2, 6, c2), (1, 1, 2, 6, c2 + 1), (1, 2, 2, 6, c2 + 1), (1, 3, 6, 6, c6 + 1),
            (1, 2, 2, 300, 5), (1, 6, 6, 300, 3)]


N_SHAPES = 15
# (noise, alpha, mu, diag_load, ref_ch)
VARIANTS = [("residual", 0.98, 0.0, 1e-3, 0), ("mix", 0.9, 0.0, 1e-3, 1), ("residual", 0.98, 1.0, 0.0, 0)]
ALL = ("out", "phi_s", "phi_n", "w", "fail", "n")


def _kw(v):
    return dict(noise=v[0], alpha=v[1], mu=v[2], diag_load=v[3], ref_ch=v[4])


def _C(M):
    from misonet_amd.beamform import cells_per_block
    return cells_per_block(M)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(shape, variant):
    return R.figures(*R.inputs(*shape), **_kw(variant))


def _run(images, mix, cuts=None, **kw):
    """the stream on the device, in one call or in the calls ``cuts`` and the rest -> dict(out, phi_s, phi_n, w, fail, n), numpy"""
    from misonet_amd.beamform import BeamformStream
    B, S, M, T, F = images.shape
    st = BeamformStream(M, S, F, B, **kw)
    outs = []
    for t0, t1 in R.pieces(T, cuts):
        outs.append(st.process(torch.from_numpy(np.ascontiguousarray(images[:, :, :, t0:t1])).cuda(),
                               torch.from_numpy(np.ascontiguousarray(mix[:, :, t0:t1])).cuda()))
    d = {k: v.cpu().numpy() for k, v in st._debug().items()}
    d["out"] = torch.cat(outs, dim=2).cpu().numpy()
    return d


def _same(a, b, what=ALL):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in what)


def _errors(got, ref):
    ext = ref["ext"]
    return (R.rel(got["out"], ref["out"]), R.rel(got["phi_s"], ext.phi_s), R.rel(got["phi_n"], ext.phi_n), R.rel(got["w"], ext.w))


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("i", range(N_SHAPES))
def test_against_restatement(i, variant):
    _need_gpu()
    shape = shapes(_C)[i]
    ref = _ref(shape, variant)
    st, bar = ref["st"], ref["bar"]
    got = _run(*R.inputs(*shape), **_kw(variant))
    e_out, e_s, e_n, e_w = _errors(got, ref)
    print(f"[obf] case {shape} {variant}: out {e_out:.3e} (bar {R.OUT_BAR:g})  Phi_s {e_s:.3e}  Phi_n {e_n:.3e}  w {e_w:.3e} "
          f"(own {ref['own']:.3e}, bar {bar:.3e})")
    B, S, M, T, F = shape
    assert bar <= R.BAR_CAP
    assert got["out"].dtype == np.complex64 and got["out"].shape == (B, S, T, F)
    assert got["phi_s"].shape == (B, S, F, M, M) and got["w"].shape == (B, S, F, M) and got["phi_s"].dtype == np.complex128
    assert np.array_equal(got["fail"], st.fail) and not st.fail.any() and np.array_equal(got["n"], st.n)
    assert R.hermitian(got["phi_s"]) and R.hermitian(got["phi_n"]), "the covariances are not exactly Hermitian"
    assert e_out <= R.OUT_BAR, e_out
    assert e_s <= bar and e_n <= bar and e_w <= bar, (e_s, e_n, e_w, bar)
    assert not R.rejected(got, ref)


@pytest.mark.parametrize("i", range(N_SHAPES))
def test_cut_invariance(i):
    """the cuts [1, 1, 2, 17, rest], and one frame per call where T <= 40: the bits of the one-call run"""
    _need_gpu()
    shape = shapes(_C)[i]
    images, mix = R.inputs(*shape)
    kw = _kw(VARIANTS[i % 3])
    whole = _run(images, mix, **kw)
    assert _same(whole, _run(images, mix, cuts=CUTS, **kw))
    if shape[3] <= 40:
        assert _same(whole, _run(images, mix, cuts=[1] * shape[3], **kw))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    images, mix = R.inputs(3, 3, 4, 50, 5)
    a, b = _run(images, mix), _run(images, mix)
    assert _same(a, b)
    one = _run(np.ascontiguousarray(images[1:2]), np.ascontiguousarray(mix[1:2]))
    assert all(np.array_equal(_bits(one[k][0]), _bits(a[k][1])) for k in ALL)


def test_buffers_that_held_nan():
    """reset writes the whole state and the call every output element: NaN in either beforehand changes no bit"""
    _need_gpu()
    from misonet_amd.beamform import BeamformStream
    B, S, M, T, F = 2, 2, 3, 20, 4
    images, mix = R.inputs(B, S, M, T, F)
    want = _run(images, mix)
    st = BeamformStream(M, S, F, B)
    st.state.fill_(0xFF)
    st.reset()
    out = torch.full((B, S, T, F), complex(float("nan"), float("nan")), dtype=torch.complex64, device="cuda")
    st.process_into(torch.from_numpy(images).cuda(), torch.from_numpy(mix).cuda(), out)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["out"] = out.cpu().numpy()
    assert _same(want, got)
    assert st.frames_seen == T and not bool(st.fail.any())
    assert st.filters().shape == (B, S, F, M) and [tuple(c.shape) for c in st.covariances()] == [(B, S, F, M, M)] * 2


def test_planted_non_finite_samples():
    """a NaN in mix (every source of that bin) and an Inf in images (that source alone), both at frame 10"""
    _need_gpu()
    B, S, M, T, F = 1, 2, 3, 40, 4
    images, mix = (a.copy() for a in R.inputs(B, S, M, T, F))
    clean = _run(images, mix)
    mix[0, 1, 10, 2] = complex(np.nan, 0.0)
    images[0, 1, 2, 10, 3] = complex(0.0, -np.inf)
    before = _run(images[:, :, :, :10], mix[:, :, :10])
    at = _run(images[:, :, :, :11], mix[:, :, :11])
    got = _run(images, mix)
    ref = R.figures(images, mix)
    want = np.zeros((B, S, F), np.int32)
    want[0, :, 2] = 1
    want[0, 1, 3] = 1
    assert np.array_equal(got["fail"], want) and np.array_equal(ref["st"].fail, want) and (got["n"] == T).all()
    assert not got["out"][0, :, 10, 2].any() and not got["out"][0, 1, 10, 3] and got["out"][0, 0, 10, 3]
    for k in ("phi_s", "phi_n", "w"):                                    # a flagged cell's state continues from the frame before
        for cell in ((0, 0, 2), (0, 1, 2), (0, 1, 3)):
            assert np.array_equal(_bits(at[k][cell]), _bits(before[k][cell])), (k, cell)
        assert not np.array_equal(_bits(at[k][0, 0, 3]), _bits(before[k][0, 0, 3])), k
    untouched = want == 0                                                # every other cell's bits are those of the clean stream
    for k in ALL:
        a, b = (np.moveaxis(d[k], 2, -1) if k == "out" else d[k] for d in (got, clean))
        assert np.array_equal(_bits(a[untouched]), _bits(b[untouched])), k
    e_out, e_s, e_n, e_w = _errors(got, ref)
    print(f"[obf] planted NaN and Inf: out {e_out:.3e}  Phi_s {e_s:.3e}  Phi_n {e_n:.3e}  w {e_w:.3e} (bar {ref['bar']:.3e})")
    assert not R.rejected(got, ref) and ref["bar"] <= R.BAR_CAP
    assert all(np.isfinite(got[k]).all() for k in ("out", "phi_s", "phi_n", "w"))


def test_source_silent_at_first():
    _need_gpu()
    images, mix = (a.copy() for a in R.inputs(1, 2, 3, 30, 3))
    images[0, 1, :, :5] = 0
    for mu in (0.0, 1.0):
        got = _run(images, mix, mu=mu)
        ref = R.figures(images, mix, mu=mu)
        print(f"[obf] silent at first, mu {mu:g}: out {R.rel(got['out'], ref['out']):.3e}  w {R.rel(got['w'], ref['ext'].w):.3e}")
        assert not got["out"][0, 1, :5].any() and got["out"][0, 1, 5:].all() and not got["fail"].any()
        assert not R.rejected(got, ref)


def test_pivot_failure():
    """images = mix: v = 0 exactly; with init = diag_load = epsi = 0, R = 0 and the first pivot is 0 in every frame"""
    _need_gpu()
    _, mix = R.inputs(1, 1, 3, 20, 3)
    images = np.ascontiguousarray(mix[:, None])
    got = _run(images, mix, init=0.0, diag_load=0.0, epsi=0.0)
    ref = R.figures(images, mix, init=0.0, diag_load=0.0, epsi=0.0)
    e_s = R.rel(got["phi_s"], ref["ext"].phi_s)
    print(f"[obf] pivot failure: fail {sorted(set(got['fail'].ravel().tolist()))}  Phi_s {e_s:.3e} (bar {ref['bar']:.3e})")
    assert (got["fail"] == 2).all() and (ref["st"].fail == 2).all() and not got["out"].any() and not got["w"].any()
    assert e_s <= ref["bar"] <= R.BAR_CAP and not got["phi_n"].any() and (got["n"] == 20).all()
    ok = _run(images, mix, init=0.0, diag_load=0.0, epsi=1e-10)
    assert not ok["fail"].any() and ok["out"].any()


@pytest.mark.parametrize("M", [2, 6])
def test_distortionless_identity(M):
    _need_gpu()
    for ref_ch in (0, 1):
        images, mix, a = R.rank_one(M, 50, 3, seed=M + ref_ch)
        from misonet_amd.beamform import BeamformStream
        st = BeamformStream(M, 1, 3, 1, ref_ch=ref_ch)
        st.process(torch.from_numpy(images).cuda(), torch.from_numpy(mix).cuda())
        w = st.filters().cpu().numpy()[0, 0]
        got = np.einsum("fm,fm->f", np.conj(w), a.astype(np.complex128))
        err = (np.abs(got - a[:, ref_ch]) / np.abs(a[:, ref_ch])).max()
        print(f"[obf] distortionless on the device, M {M} ref {ref_ch}: {err:.3e}")
        assert err <= 1e-9 and not bool(st.fail.any())


def test_captured_graph_replayed_over_three_blocks():
    """one captured misonet_obf of T = 16, replayed over three successive blocks = the eager stream, bit for bit (a single stream
    of launches: no parallel branches in the graph)"""
    _need_gpu()
    from misonet_amd.beamform import BeamformStream
    B, S, M, T, F = 1, 4, 4, 48, 5
    images, mix = R.inputs(B, S, M, T, F)
    want = _run(images, mix, cuts=[16, 16])
    st = BeamformStream(M, S, F, B)
    x = torch.zeros((B, S, M, 16, F), dtype=torch.complex64, device="cuda")
    y = torch.zeros((B, M, 16, F), dtype=torch.complex64, device="cuda")
    out = torch.empty((B, S, 16, F), dtype=torch.complex64, device="cuda")
    xs = [torch.from_numpy(np.ascontiguousarray(images[:, :, :, i * 16:(i + 1) * 16])).cuda() for i in range(3)]
    ys = [torch.from_numpy(np.ascontiguousarray(mix[:, :, i * 16:(i + 1) * 16])).cuda() for i in range(3)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(stream):
        st.process_into(x, y, out)                                       # warm-up on the side stream, then a fresh state
        st.reset()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            st.process_into(x, y, out)
        for xb, yb in zip(xs, ys):
            x.copy_(xb)
            y.copy_(yb)
            graph.replay()
            outs.append(out.clone())
        stream.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["out"] = torch.cat(outs, dim=2).cpu().numpy()
    assert _same(want, got)


def test_composition_behind_online_wpe_and_online_auxiva():
    """DereverbStream -> SeparateStream(images=True) -> BeamformStream on a (1, 4, 60, 9) stream cut in three, against the
    restatement chain owpe_ref -> oiva_ref -> obf_ref; every stage within its bars"""
    _need_gpu()
    import oiva_ref
    import owpe_ref
    from misonet_amd.beamform import BeamformStream
    from misonet_amd.blind import SeparateStream
    from misonet_amd.dereverb import DereverbStream
    B, M, T, F = 1, 4, 60, 9
    mix = oiva_ref.to_stream(iva_ref.sparse_mixture(B, M, M, T, F, seed=B + M + T + F)[0])
    x = torch.from_numpy(mix).cuda()
    d, s, b = DereverbStream(M, F, B, taps=3, delay=2), SeparateStream(M, F, B), BeamformStream(M, M, F, B)
    ders, imgs, outs = [], [], []
    for t in range(0, T, 20):
        der = d.process(x[:, :, t:t + 20].contiguous())
        est, img = s.process(der, images=True)
        outs.append(b.process(img, der))
        ders.append(der)
        imgs.append(img)
    der, img, out = torch.cat(ders, 2).cpu().numpy(), torch.cat(imgs, 3).cpu().numpy(), torch.cat(outs, 2).cpu().numpy()
    r_der = owpe_ref.owpe(mix, taps=3, delay=2)[0]
    r_img = oiva_ref.oiva(r_der)[1]
    chain = R.obf(r_img, r_der)[0]
    # out against the whole restatement chain; the beamformer's state against the restatement on the inputs the stage saw (the
    # device's der and images: the chain's own bits wherever the two stages in front return the restatement's complex64)
    ref = R.figures(img, der)
    got = {k: v.cpu().numpy() for k, v in b._debug().items()}
    got["out"] = out
    e_der, e_img, e_chain = R.rel(der, r_der), R.rel(img, r_img), R.rel(out, chain)
    e_out, e_s, e_n, e_w = _errors(got, ref)
    print(f"[obf] composition: owpe {e_der:.3e} oiva images {e_img:.3e} out against the chain {e_chain:.3e} (bar {R.OUT_BAR:g})  "
          f"out {e_out:.3e}  Phi_s {e_s:.3e}  Phi_n {e_n:.3e}  w {e_w:.3e} (bar {ref['bar']:.3e})")
    assert e_der <= R.OUT_BAR and e_img <= R.OUT_BAR and e_chain <= R.OUT_BAR
    assert ref["bar"] <= R.BAR_CAP and not got["fail"].any() and not R.rejected(got, ref)


def test_numpy_in_numpy_out_and_the_library_refuses():
    _need_gpu()
    import ctypes as C
    from misonet_amd import _lib
    from misonet_amd.beamform import BeamformStream, beamform_online
    images, mix = R.inputs(1, 2, 2, 40, 5)
    out = beamform_online(images, mix)
    assert isinstance(out, torch.Tensor) and out.device.type == "cpu" and out.dtype == torch.complex64 and out.shape == (1, 2, 40, 5)
    assert R.rel(out.numpy(), R.obf(images, mix)[0]) <= R.OUT_BAR
    dev, dbg = beamform_online(torch.from_numpy(images).cuda(), torch.from_numpy(mix).cuda(), return_debug=True)
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(out.numpy())) and (dbg["n"] == 40).all()
    st = BeamformStream(2, 2, 5, 1)
    with pytest.raises(ValueError):
        st.process(images[..., :4], mix[..., :4])
    L = _lib.lib()
    x, y = torch.from_numpy(images).cuda(), torch.from_numpy(mix).cuda()
    o = torch.empty((1, 2, 40, 5), dtype=torch.complex64, device="cuda")
    s = _lib.stream_ptr(x.device)
    n = st.state.numel()
    call = lambda mp, ip, T, op, nb: L.misonet_obf(mp, ip, 1, 2, 2, T, 5, C.byref(st._c), op, st.state.data_ptr(), nb, s)
    assert call(y.data_ptr(), x.data_ptr(), 40, y.data_ptr(), n) == _lib.EINVAL
    assert call(y.data_ptr(), x.data_ptr(), 40, x.data_ptr(), n) == _lib.EINVAL
    assert call(y.data_ptr(), x.data_ptr(), 40, o.data_ptr(), n - 1) == _lib.ENOMEM
    assert call(y.data_ptr(), x.data_ptr(), 0, o.data_ptr(), n) == _lib.EINVAL
    assert st.frames_seen == 0


def test_recording_path():
    """separate_recording(online=True, beamform=OnlineBeamformer()) on 1 s of the six-microphone recording: int16 [S, L], not the
    rows of beamform=False, the same bytes twice, and the iSTFT of the stream's rows at the indices the separation's power picks"""
    _need_gpu()
    import dataclasses
    from misonet_amd import stft as S
    from misonet_amd.beamform import BeamformStream, OnlineBeamformer
    from misonet_amd.blind import BlindSeparator, OnlineAuxIVA, SeparateStream
    wav, _, fs = iva_ref.g8_sample()
    wav = np.ascontiguousarray(wav[:fs])
    sep = BlindSeparator(num_spks=2, num_ch=2, ref_ch=1)
    a = sep.separate_recording(wav, online=True, beamform=OnlineBeamformer())
    b = sep.separate_recording(wav, online=True, beamform=OnlineBeamformer())
    plain = sep.separate_recording(wav, online=True, beamform=False)
    assert a.dtype == np.int16 and a.shape == (2, fs) and a.any() and a.tobytes() == b.tobytes()
    assert a.tobytes() != plain.tobytes() and plain.tobytes() == sep.separate_recording(wav, online=True).tobytes()
    # by hand: the same chain, the instance's ref_ch replaced by the separator's
    mics, obs = sep._select_mics(wav, None)
    sig = torch.from_numpy(np.ascontiguousarray(obs[:, mics])).cuda()
    sig = torch.nn.functional.pad(sig, (0, 0, 0, (-fs) % S.HOP))[None].contiguous()
    spec = S.stft_hip(sig)
    M, F = spec.shape[1], spec.shape[3]
    est, img = SeparateStream(M, F, 1, **dataclasses.asdict(OnlineAuxIVA(ref_ch=1))).process(spec, images=True)
    out = BeamformStream(M, M, F, 1, ref_ch=1).process(img, spec)
    rows = sep._online_pick(est[0])
    assert torch.equal(est[0][rows], sep._online_rows(spec, OnlineAuxIVA(ref_ch=1), None))
    want = S.istft_int16(out[0][rows].contiguous())[:, :fs].cpu().numpy()
    assert a.tobytes() == np.ascontiguousarray(want).tobytes()
    d = sep.separate_recording(wav, online=True, dereverb=dict(taps=3), beamform=OnlineBeamformer(noise="mix", alpha=0.9))
    assert d.shape == (2, fs) and d.tobytes() != a.tobytes()
    with pytest.raises(ValueError):
        sep.separate_recording(wav, beamform=OnlineBeamformer())            # the online beamformer belongs to the online path
    with pytest.raises(ValueError):
        sep.separate_recording(wav, beamform=True, online=True)             # as before: the other beamformers are block algorithms
