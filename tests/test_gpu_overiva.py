"""GPU tests of the online AuxIVA for fewer sources than microphones (csrc/overiva.hip, ``SeparateStream(..., num_src=K)``)
against the float64 NumPy restatement of tests/overiva_ref.py: est, images, Ws, J, V, C, fail and n at all 28 pairs (M, K), at
F = P - 1, P, P + 1 and 2 P + 1 around the bins one workgroup covers at once (P = ``misonet_overiva_bins_per_pass``), on a single
frame of a single bin and on a long stream; that the bits do not depend on how the stream is cut into calls; bit reproducibility
and independence of the batch; buffers that held NaN; a planted non-finite sample; an all-zero bin; a duplicated microphone; a
captured graph; that ``num_src`` None or M is the determined stream as it was; the chain of ``StreamSeparator`` and the
recording path with ``num_src`` set.

Bars (``overiva_ref``).  est and images: rel-L2 <= 2.4e-7 = 4 x 2^-24, one complex64 rounding of a float64 result.  Ws, J, V and
C, against the clongdouble run of the restatement: 100 x the larger of the rel-L2 distances float64 - clongdouble and float64 -
reversed summation order of the restatement on that case, never below 1e-12 and, for every case here, not above 1e-6
(tests/test_overiva.py checks that on the CPU).  C and every V_k exactly Hermitian; fail and n equal.  The invariants of the
definition: |[J, -I] C Ws^H| <= 1e-12, |Re(w_k^H V_k w_k) - 1| <= 1e-9, |W A - [I; 0]| <= 1e-9.  tests/test_overiva.py shows that
each planted mistake misses these bars.  The module prints every figure (``[overiva] ...``); LAB.md has them.

Measured on an MI355X: est and images equal the restatement's complex64 on every case but the 300-frame gauss one (1.7e-10); Ws
within 3.7e-11, J 1.9e-10, V 9.9e-12 and C 2.6e-16 rel-L2 of the clongdouble run (all but C on that case; own 2.7e-10 there);
|[J, -I] C Ws^H| <= 2.2e-15; |w^H V w - 1| <= 1.5e-12; |W A - [I; 0]| <= 7.9e-16."""
import functools

import numpy as np
import pytest
import torch

import overiva_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

N_EDGES = 8


def _P(M, K):
    from misonet_amd.blind import bins_per_pass
    return bins_per_pass(M, K)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize % 8 == 0 else a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    return R.case_inputs(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, variant):
    return R.figures(_inputs(shape), shape[2], model=variant[0], alpha=variant[1], ref_ch=R.ref_ch_of(shape, variant))


def _run(mix, K, cuts=None, images=True, **kw):
    """the stream on the device, in one call or in the calls ``cuts`` and the rest -> dict(est, images, Ws, J, V, C, fail, n)"""
    from misonet_amd.blind import SeparateStream
    B, M, T, F = mix.shape
    st = SeparateStream(M, F, B, num_src=K, **kw)
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


ALL = ("est", "images") + R.PARTS + ("fail", "n")


def _same(a, b, what=ALL):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in what)


def _against(shape, variant):
    model, alpha, images, _ = variant
    K, ref_ch = shape[2], R.ref_ch_of(shape, variant)
    ref = _ref(shape, variant)
    st, ext, bar = ref["st"], ref["ext"], ref["bar"]
    got = _run(_inputs(shape), K, images=images, model=model, alpha=alpha, ref_ch=ref_ch)
    e_est = R.rel(got["est"], ref["est"])
    e_img = R.rel(got["images"], ref["images"]) if images else 0.0
    e = {p: R.rel(got[p], getattr(ext, p)) for p in R.PARTS}
    orth = R.orthogonality_error(got["Ws"], got["J"], got["C"])
    unit, inv = R.unit_norm_error(got["Ws"], got["V"]), R.inverse_error(got["Ws"], got["J"])
    print(f"[overiva] case {shape} {model} alpha {alpha:g} ref {ref_ch}: est {e_est:.3e} images {e_img:.3e} (bar {R.OUT_BAR:g})  "
          + "  ".join(f"{p} {v:.3e}" for p, v in e.items()) + f" (own {ref['own']:.3e}, bar {bar:.3e})  |[J, -I] C Ws^H| {orth:.3e}  "
          f"|w^H V w - 1| {unit:.3e}  |W A - [I; 0]| {inv:.3e}")
    assert bar <= R.BAR_CAP
    assert got["est"].dtype == np.complex64 and got["est"].shape == ref["est"].shape
    assert not images or got["images"].shape == ref["images"].shape
    assert np.array_equal(got["fail"], st.fail) and not st.fail.any() and np.array_equal(got["n"], st.n)
    assert R.hermitian(got["V"]) and R.hermitian(got["C"]), "V or C is not exactly Hermitian"
    assert e_est <= R.OUT_BAR and e_img <= R.OUT_BAR, (e_est, e_img)
    assert all(v <= bar for v in e.values()), (e, bar)
    assert orth <= 1e-12 and unit <= 1e-9 and inv <= 1e-9, (orth, unit, inv)
    if ref_ch >= K and images:                                                      # est is the image at ref_ch, a background microphone
        assert np.array_equal(_bits(got["est"]), _bits(got["images"][:, :, ref_ch]))


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "x".join(map(str, R.CASES[i][0])))
def test_against_restatement(i):
    _need_gpu()
    shape, variants = R.CASES[i]
    for v in variants:
        _against(shape, v)


@pytest.mark.parametrize("i", range(N_EDGES))
def test_against_restatement_around_a_pass(i):
    _need_gpu()
    edges = R.edge_cases(_P)
    assert len(edges) == N_EDGES
    shape, (v,) = edges[i]
    _against(shape, v)


@pytest.mark.parametrize("shape", [(2, 6, 2, 40, 5), (1, 3, 2, 30, 2), (1, 8, 7, 30, 2), (1, 5, 1, 30, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_cut_invariance(shape):
    """the cuts [1, 1, 2, 17, rest]: the bits of the one-call run"""
    _need_gpu()
    whole = _run(_inputs(shape), shape[2], alpha=0.96)
    cut = _run(_inputs(shape), shape[2], cuts=[1, 1, 2, 17], alpha=0.96)
    assert _same(whole, cut)


@pytest.mark.parametrize("shape", [(2, 6, 2, 12, 5), (1, 4, 3, 12, 2)], ids=lambda s: "x".join(map(str, s)))
def test_one_frame_per_call(shape):
    _need_gpu()
    mix = R.inputs(*shape)
    assert _same(_run(mix, shape[2], model="laplace"), _run(mix, shape[2], cuts=[1] * shape[3], model="laplace"))


def test_bit_reproducible_and_batch_independent():
    _need_gpu()
    mix = R.inputs(3, 6, 2, 50, 5)
    a, b = _run(mix, 2), _run(mix, 2)
    assert _same(a, b)
    one = _run(np.ascontiguousarray(mix[1:2]), 2)
    assert all(np.array_equal(_bits(one[k][0]), _bits(a[k][1])) for k in ALL)


def test_buffers_that_held_nan():
    """reset writes the whole state and the call every output element: NaN in either beforehand changes no bit"""
    _need_gpu()
    from misonet_amd.blind import SeparateStream
    B, M, K, T, F = 2, 5, 2, 20, 4
    mix = R.inputs(B, M, K, T, F)
    want = _run(mix, K)
    st = SeparateStream(M, F, B, num_src=K)
    st.state.fill_(0xFF)
    st.reset()
    x = torch.from_numpy(mix).cuda()
    nan = complex(float("nan"), float("nan"))
    est = torch.full((B, K, T, F), nan, dtype=torch.complex64, device="cuda")
    img = torch.full((B, K, M, T, F), nan, dtype=torch.complex64, device="cuda")
    st.process_into(x, est, img)
    got = {k: v.cpu().numpy() for k, v in st._debug().items()}
    got["est"], got["images"] = est.cpu().numpy(), img.cpu().numpy()
    assert _same(want, got)
    assert st.frames_seen == T and not bool(st.fail.any())
    assert st.demixing().shape == (B, F, K, M) and st.covariance().shape == (B, F, K, M, M)
    assert st.background().shape == (B, F, M - K, K) and st.mixture_covariance().shape == (B, F, M, M)
    assert np.array_equal(st.background().cpu().numpy(), got["J"]) and np.array_equal(st.mixture_covariance().cpu().numpy(), got["C"])


def test_planted_non_finite_sample():
    _need_gpu()
    B, M, K, T, F = 1, 4, 2, 40, 4
    mix = R.inputs(B, M, K, T, F).copy()
    mix[0, 1, 10, 2] = complex(np.nan, 0.0)
    before = _run(mix[:, :, :10], K)
    at = _run(mix[:, :, :11], K)
    got = _run(mix, K)
    ref = R.figures(mix, K)
    want = np.zeros((B, F), np.int32)
    want[0, 2] = 1
    assert np.array_equal(got["fail"], want) and np.array_equal(ref["st"].fail, want) and (got["n"] == T).all()
    assert not got["est"][0, :, 10, 2].any() and not got["images"][0, :, :, 10, 2].any()
    for k in R.PARTS:                                                # that bin's state is unchanged by the frame, its neighbour's not
        assert np.array_equal(_bits(at[k][0, 2]), _bits(before[k][0, 2])), k
        assert not np.array_equal(_bits(at[k][0, 1]), _bits(before[k][0, 1])), k
    e_est, e_img = R.rel(got["est"], ref["est"]), R.rel(got["images"], ref["images"])
    e = {p: R.rel(got[p], getattr(ref["ext"], p)) for p in R.PARTS}
    print(f"[overiva] planted NaN: est {e_est:.3e} images {e_img:.3e}  " + "  ".join(f"{p} {v:.3e}" for p, v in e.items())
          + f" (bar {ref['bar']:.3e})")
    assert e_est <= R.OUT_BAR and e_img <= R.OUT_BAR and all(v <= ref["bar"] for v in e.values()) and ref["bar"] <= R.BAR_CAP
    assert all(np.isfinite(got[k]).all() for k in ("est", "images") + R.PARTS)


def test_all_zero_bin():
    _need_gpu()
    mix = R.inputs(1, 4, 2, 40, 4).copy()
    mix[..., 1] = 0
    got = _run(mix, 2)
    _, _, ref = R.overiva(mix, 2)
    assert np.array_equal(got["fail"], ref.fail) and not (got["fail"] & 1).any()
    assert all(np.isfinite(got[k]).all() for k in ("est", "images") + R.PARTS) and not got["est"][..., 1].any()


def test_duplicated_microphone():
    """Identical microphones and a V far below the data (init 1e-300): the covariances round to exactly singular rank-one
    matrices, eliminations meet a zero pivot, updates are dropped: flags as the restatement's, nothing is NaN, the state stays
    finite and Hermitian"""
    _need_gpu()
    mix = R.inputs(1, 3, 1, 20, 3).copy()
    mix[:, 1] = mix[:, 0]
    mix[:, 2] = mix[:, 0]
    got = _run(mix, 1, init=1e-300)
    _, _, ref = R.overiva(mix, 1, init=1e-300)
    print(f"[overiva] duplicated microphone: fail {sorted(set(got['fail'].ravel().tolist()))} (restatement "
          f"{sorted(set(ref.fail.ravel().tolist()))})")
    assert np.array_equal(got["fail"], ref.fail) and ref.fail.any() and not (got["fail"] & 1).any()
    assert all(np.isfinite(got[k]).all() for k in ("est", "images") + R.PARTS)
    assert R.hermitian(got["V"]) and R.hermitian(got["C"])


def test_captured_graph_replayed_over_three_blocks():
    """one captured misonet_overiva of T = 8, replayed over three successive blocks = three eager calls, bit for bit (a single
    stream of launches: no parallel branches in the graph)"""
    _need_gpu()
    from misonet_amd.blind import SeparateStream
    B, M, K, T, F = 1, 6, 2, 24, 5
    mix = R.inputs(B, M, K, T, F)
    want = _run(mix, K, cuts=[8, 8])
    st = SeparateStream(M, F, B, num_src=K)
    x = torch.zeros((B, M, 8, F), dtype=torch.complex64, device="cuda")
    est = torch.empty((B, K, 8, F), dtype=torch.complex64, device="cuda")
    img = torch.empty((B, K, M, 8, F), dtype=torch.complex64, device="cuda")
    blocks = [torch.from_numpy(np.ascontiguousarray(mix[:, :, i * 8:(i + 1) * 8])).cuda() for i in range(3)]
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


def test_num_src_none_or_m_is_the_determined_stream():
    """``SeparateStream(6, num_src=6)`` and ``num_src=None`` are today's stream, to the bit, and its state's parts"""
    _need_gpu()
    import oiva_ref
    from misonet_amd.blind import SeparateStream, auxiva_online, bins_per_pass
    mix = torch.from_numpy(R.inputs(1, 6, 6, 20, 5)).cuda()
    runs = []
    for kw in ({}, dict(num_src=None), dict(num_src=6)):
        st = SeparateStream(6, 5, 1, **kw)
        est, img = st.process(mix, images=True)
        d = {k: v.cpu().numpy() for k, v in st._debug().items()}
        assert sorted(d) == ["V", "W", "fail", "n"] and est.shape == (1, 6, 20, 5) and img.shape == (1, 6, 6, 20, 5)
        d["est"], d["images"] = est.cpu().numpy(), img.cpu().numpy()
        runs.append(d)
        with pytest.raises(ValueError):
            st.background()
    keys = ("est", "images", "W", "V", "fail", "n")
    assert _same(runs[0], runs[1], keys) and _same(runs[0], runs[2], keys)
    ref_est, ref_img, _ = oiva_ref.oiva(mix.cpu().numpy())
    assert R.rel(runs[2]["est"], ref_est) <= R.OUT_BAR and R.rel(runs[2]["images"], ref_img) <= R.OUT_BAR
    assert bins_per_pass(6) == bins_per_pass(6, 6) == bins_per_pass(6, None) and bins_per_pass(6, 2) == _P(6, 2)
    one = auxiva_online(mix, num_src=2, images=True, return_debug=True)
    assert one[0].shape == (1, 2, 20, 5) and one[1].shape == (1, 2, 6, 20, 5) and sorted(one[2]) == ["C", "J", "V", "Ws", "fail", "n"]
    assert np.array_equal(_bits(one[0].cpu().numpy()), _bits(_run(mix.cpu().numpy(), 2)["est"]))


@functools.lru_cache(maxsize=None)
def _recording():
    """two sparse sources at six microphones, 64 * 40 + 17 samples: float32 [L, 6]"""
    rng = np.random.default_rng(670)
    L = 64 * 40 + 17
    env = np.repeat(rng.random((2, L // 256 + 1)) < 0.6, 256, axis=1)[:, :L]
    src = rng.standard_normal((2, L)) * env * np.array([[0.2], [0.14]])
    wav = np.zeros((L, 6))
    for m in range(6):
        for s in range(2):
            h = rng.standard_normal(8) * 0.5 ** np.arange(8)
            wav[:, m] += np.convolve(src[s], h)[:L]
    return np.ascontiguousarray((wav + 1e-3 * rng.standard_normal((L, 6))).astype(np.float32))


def test_stream_separator_with_num_src():
    """StreamSeparator(6, separate=dict(num_src=2), beamform=OnlineBeamformer()): two rows, the same int16 bits in blocks of 64, of
    1000 and whole, and those of the stages called one after the other"""
    _need_gpu()
    from misonet_amd import stft as S
    from misonet_amd.beamform import BeamformStream, OnlineBeamformer
    from misonet_amd.blind import SeparateStream
    from misonet_amd.stream import StreamSeparator
    wav = _recording()
    L = wav.shape[0]
    sig = torch.nn.functional.pad(torch.from_numpy(wav).cuda(), (0, 0, 0, (-L) % 64))[None].contiguous()
    spec = S.stft_hip(sig)
    s, b = SeparateStream(6, 129, 1, num_src=2), BeamformStream(6, 2, 129, 1)
    _est, img = s.process(spec, images=True)
    full = S.istft_int16(b.process(img, spec)[0].contiguous())
    assert not bool(s.fail.any()) and not bool(b.fail.any()) and int(full.abs().max()) > 100
    sep = StreamSeparator(6, separate=dict(num_src=2), beamform=OnlineBeamformer())
    assert sep.rows == [0, 1] and sep.num_src == 2
    for block in (64, 1000, 0):
        sep.reset()
        out = [sep.process(sig[:, a:a + block]) for a in range(0, sig.shape[1], block)] if block else []
        out.append(sep.flush() if block else sep.flush(sig))
        got = torch.cat(out, dim=2)
        assert got.dtype == torch.int16 and got.shape == (1, 2, full.shape[1]), (block, got.shape)
        assert torch.equal(got[0], full), block
        assert not any(bool(v.any()) for v in sep.fail.values())
    one = StreamSeparator(6, separate=dict(num_src=2), rows=[1])
    got = torch.cat([one.process(sig), one.flush()], dim=2)
    plain = S.istft_int16(SeparateStream(6, 129, 1, num_src=2).process(spec)[0].contiguous())
    assert got.shape == (1, 1, plain.shape[1]) and torch.equal(got[0, 0], plain[1])


def test_recording_path_makes_no_choice():
    """separate_recording(online=dict(num_src=2)) at six microphones and two speakers: two waves, the rows of the stream in its
    order, the strongest-rows pick never called; num_src=3 picks two of three; num_src=1 is refused"""
    _need_gpu()
    from misonet_amd import stft as S
    from misonet_amd.blind import BlindSeparator, SeparateStream
    wav = _recording()
    L = wav.shape[0]
    sep = BlindSeparator(num_spks=2, num_ch=6)
    picks = []
    pick = sep._online_pick
    sep._online_pick = lambda est: picks.append(1) or pick(est)
    a = sep.separate_recording(wav, online=dict(num_src=2))
    assert a.dtype == np.int16 and a.shape == (2, L) and a.any() and not picks
    sig = torch.nn.functional.pad(torch.from_numpy(wav).cuda(), (0, 0, 0, (-L) % 64))[None].contiguous()
    est = SeparateStream(6, 129, 1, num_src=2).process(S.stft_hip(sig))[0]
    assert np.array_equal(a, S.istft_int16(est.contiguous())[:, :L].cpu().numpy())
    c = sep.separate_recording(wav, online=dict(num_src=3))
    assert c.shape == (2, L) and picks == [1]
    with pytest.raises(ValueError):
        sep.separate_recording(wav, online=dict(num_src=1))
    with pytest.raises(ValueError):
        sep.separate_recording(wav, online=dict(num_src=7))


def test_refused_arguments_raise_before_any_launch():
    _need_gpu()
    import ctypes as C
    from misonet_amd import _lib
    from misonet_amd.blind import SeparateStream
    mix = R.inputs(1, 3, 2, 40, 5)
    st = SeparateStream(3, 5, 1, num_src=2)
    with pytest.raises(ValueError):
        st.process(mix[:, :, :, :4])
    with pytest.raises(ValueError):
        st.process(mix[:, :2])
    L = _lib.lib()
    x = torch.from_numpy(mix).cuda()
    y = torch.empty((1, 2, 40, 5), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        st.process_into(x, torch.empty_like(x))                          # est has K rows, not M
    s = _lib.stream_ptr(x.device)
    n = st.state.numel()
    args = lambda K, T, out, nb: (x.data_ptr(), 1, 3, K, T, 5, C.byref(st._c), out, None, st.state.data_ptr(), nb, s)
    assert L.misonet_overiva(*args(2, 40, x.data_ptr(), n)) == _lib.EINVAL
    assert L.misonet_overiva(*args(2, 40, y.data_ptr(), n - 1)) == _lib.ENOMEM
    assert L.misonet_overiva(*args(2, 0, y.data_ptr(), n)) == _lib.EINVAL
    assert L.misonet_overiva(*args(3, 40, y.data_ptr(), n)) == _lib.EINVAL
    assert L.misonet_overiva(*args(0, 40, y.data_ptr(), n)) == _lib.EINVAL
    assert st.frames_seen == 0 and not bool(st.fail.any())
