"""GPU tests of the streaming front end (csrc/stft.hip ``stft_stream_k`` / ``istft_stream_k``, ``misonet_amd.stft.StftStream`` /
``IstftStream``, ``misonet_amd.stream.StreamSeparator``).  No tolerance appears here: every comparison is exact equality, against
the offline kernels (``stft_hip``, ``istft``, ``istft_int16`` -- whose float64 accuracy tests/test_gpu_stft.py holds) or against
the uncut stream.  The streams are cut all at once, in hops, in single samples (frames), and at seeded random lengths around the
hop, the frame and the 32- / 64-frame tiles; the flush carries the last block or none.  Beyond that: independence of the batch and
reproducibility, buffers that held NaN, calls that emit nothing, a captured graph replayed over three blocks, the whole chain
against the one-shot path of the recursions, and misuse."""
import functools

import numpy as np
import pytest
import torch

import iva_ref
import stream_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

BM = [(1, 1), (1, 6), (3, 2), (2, 8)]
LENGTHS = [1, 63, 64, 65, 128, 129, 64 * 31, 64 * 33 + 5, 64 * 65, 64 * 130 + 63]
ROWS = [1, 3, 12]
FRAMES = [2, 3, 4, 5, 62, 63, 64, 65, 66, 123, 130]
SCUTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
FCUTS = (1, 2, 3, 4, 60, 61, 62, 64, 65)


def _random_cuts(total, choices, seed):
    r, out = np.random.default_rng(seed), []
    while sum(out) < total:
        out.append(int(r.choice(choices)))
    return out


@functools.lru_cache(maxsize=None)
def _wave(B, L, M):
    """float32 [B, L, M] on the device, and stft_hip of it: computed once, never written to"""
    x = torch.from_numpy((np.random.default_rng(B + 10 * L + M).standard_normal((B, L, M)) * 0.1).astype(np.float32)).cuda()
    from misonet_amd.stft import stft_hip
    return x, stft_hip(x)


@functools.lru_cache(maxsize=None)
def _spec(Rr, T):
    """complex64 [Rr, T, 129] on the device at a peak near 0.1 of full scale, and both offline forms of its iSTFT"""
    from misonet_amd import stft as S
    wav = np.random.default_rng(100 * Rr + T).standard_normal((Rr, 64 * (T - 1))) * 0.03
    X = torch.from_numpy(R.stft(wav.T).astype(np.complex64)).cuda().contiguous()                # [Rr, T, 129]
    assert X.shape == (Rr, T, 129)
    f32, i16 = S.istft(X), S.istft_int16(X)
    assert f32.dtype == torch.float32 and i16.dtype == torch.int16 and 0.05 < float(f32.abs().max()) < 0.3
    return X, f32, i16


def _bits(t):
    return torch.view_as_real(t) if t.is_complex() else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _stft_stream(x, cuts, flush_with_block=True, st=None):
    from misonet_amd.stft import StftStream
    B, L, M = x.shape
    st = StftStream(M, B) if st is None else st.reset()
    pc = R.pieces(L, cuts)
    out = []
    for i, (a, b) in enumerate(pc):
        last = flush_with_block and i == len(pc) - 1
        out.append(st.flush(x[:, a:b]) if last else st.process(x[:, a:b]))
    if not flush_with_block:
        out.append(st.flush())
    assert st.samples_seen == L and st.frames_out == L // 64 + 1
    return torch.cat(out, dim=2)


def _istft_stream(X, cuts, int16, flush_with_block=True):
    from misonet_amd.stft import IstftStream
    Rr, T, _ = X.shape
    st = IstftStream(Rr, int16=int16)
    pc = R.pieces(T, cuts)
    out = []
    for i, (a, b) in enumerate(pc):
        last = flush_with_block and i == len(pc) - 1
        out.append(st.flush(X[:, a:b]) if last else st.process(X[:, a:b]))
    if not flush_with_block:
        out.append(st.flush())
    assert st.frames_seen == T and st.samples_out == 64 * (T - 1)
    return torch.cat(out, dim=1)


# ---- the two transforms against the offline kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("B,M", BM)
def test_stft_stream_equals_offline_bit_for_bit(B, M, L):
    _need_gpu()
    x, want = _wave(B, L, M)
    assert want.shape == (B, M, L // 64 + 1, 129)
    cutsets = [[L], [64], _random_cuts(L, SCUTS, 7 * L + M), _random_cuts(L, SCUTS, 11 * L + B)]
    if L <= 200:
        cutsets.append([1])
    for cuts in cutsets:
        for with_block in (True, False):
            got = _stft_stream(x, cuts, with_block)
            assert _same(got, want), (B, M, L, cuts, with_block)


@pytest.mark.parametrize("int16", [False, True])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("Rr", ROWS)
def test_istft_stream_equals_offline_bit_for_bit(Rr, T, int16):
    _need_gpu()
    X, f32, i16 = _spec(Rr, T)
    want = i16 if int16 else f32
    if int16:
        assert int(want.abs().max()) > 1000
    for cuts in ([T], [1], _random_cuts(T, FCUTS, 5 * T + Rr), _random_cuts(T, FCUTS, 13 * T + Rr)):
        for with_block in (True, False):
            got = _istft_stream(X, cuts, int16, with_block)
            assert _same(got, want), (Rr, T, int16, cuts, with_block)


def test_a_stream_flushed_with_fewer_than_two_frames_emits_nothing():
    _need_gpu()
    from misonet_amd.stft import IstftStream
    X = _spec(3, 4)[0]
    for T in (0, 1):
        st = IstftStream(3)
        out = st.flush(X[:, :T]) if T else st.flush()
        assert out.shape == (3, 0) and st.samples_out == 0
    st = IstftStream(3)
    assert st.process(X[:, :1]).shape == (3, 0) and st.flush().shape == (3, 0)


def test_leading_axes_and_two_dimensional_blocks():
    _need_gpu()
    from misonet_amd.stft import IstftStream, StftStream
    x, want = _wave(1, 64 * 5 + 17, 6)
    st = StftStream(6)
    got = torch.cat([st.process(x[0, :100]), st.flush(x[0, 100:])], dim=2)                      # [n, M] when batch == 1
    assert _same(got, want)
    X, f32, _ = _spec(12, 5)
    st = IstftStream(12)
    Y = X.reshape(2, 3, 2, 5, 129)
    got = torch.cat([st.process(Y[..., :3, :]), st.flush(Y[..., 3:, :])], dim=-1)
    assert got.shape == (2, 3, 2, 64 * 4) and _same(got.reshape(12, -1), f32)


# ---- independence of the batch, reproducibility, NaN ----------------------------------------------------------------------------
def test_batch_independence_and_reproducibility():
    _need_gpu()
    x, _ = _wave(3, 64 * 33 + 5, 2)
    cuts = [257, 64, 1, 1000]
    a, b = _stft_stream(x, cuts), _stft_stream(x, cuts)
    assert _same(a, b)
    for i in range(3):
        assert _same(_stft_stream(x[i:i + 1].contiguous(), cuts), a[i:i + 1]), i
    X, _, _ = _spec(12, 66)
    for int16 in (False, True):
        a, b = _istft_stream(X, [3, 61, 1], int16), _istft_stream(X, [3, 61, 1], int16)
        assert _same(a, b)
        for i in (0, 5, 11):
            assert _same(_istft_stream(X[i:i + 1].contiguous(), [3, 61, 1], int16), a[i:i + 1]), i


def test_buffers_that_held_nan():
    """outputs and state pre-filled with NaN before reset: reset writes every byte of the state, a call every element of its
    output"""
    _need_gpu()
    from misonet_amd.stft import IstftStream, StftStream
    x, want = _wave(3, 64 * 33 + 5, 2)
    st = StftStream(2, 3)
    st.state.view(torch.float32).fill_(float("nan"))
    st.reset()
    outs = []
    for i, (a, b) in enumerate(R.pieces(x.shape[1], [300, 64, 1, 1000])):
        out = torch.full((3, 2, st.frames(b - a), 129), float("nan"), dtype=torch.complex64, device="cuda")
        st.process_into(x[:, a:b].contiguous(), out)
        outs.append(out)
    out = torch.full((3, 2, st.frames(0, True), 129), float("nan"), dtype=torch.complex64, device="cuda")
    outs.append(st.process_into(x[:, :0].contiguous(), out, flush=True))
    got = torch.cat(outs, dim=2)
    assert bool(torch.isfinite(torch.view_as_real(got)).all()) and _same(got, want)
    X, f32, i16 = _spec(3, 66)
    for int16, want in ((False, f32), (True, i16)):
        st = IstftStream(3, int16=int16)
        st.state.view(torch.float32).fill_(float("nan"))
        st.reset()
        outs = []
        for a, b in R.pieces(66, [1, 2, 40]):
            out = (torch.full((3, 64 * st.hops(b - a)), -12345, dtype=torch.int16, device="cuda") if int16 else
                   torch.full((3, 64 * st.hops(b - a)), float("nan"), dtype=torch.float32, device="cuda"))
            st.process_into(X[:, a:b].contiguous(), out)
            outs.append(out)
        outs.append(st.flush())
        got = torch.cat(outs, dim=1)
        assert _same(got, want)
        assert bool(torch.isfinite(got.float()).all())


# ---- calls that emit nothing ------------------------------------------------------------------------------------------------------
def test_zero_frame_calls():
    _need_gpu()
    from misonet_amd.stft import StftStream, stft_hip
    from misonet_amd.stream import StreamSeparator
    x, want = _wave(1, 64 * 5 + 17, 2)
    st = StftStream(2)
    for i in range(3):
        out = st.process(x[:, 20 * i:20 * (i + 1)])
        assert out.shape == (1, 2, 0, 129) and out.dtype == torch.complex64
    assert (st.samples_seen, st.frames_out) == (60, 0)
    fourth = st.process(x[:, 60:260])                                    # 260 samples: frames 0, 1, 2 are complete
    assert fourth.shape == (1, 2, 3, 129) and _same(fourth, want[:, :, :3].contiguous())
    assert _same(torch.cat([fourth, st.flush(x[:, 260:])], dim=2), want)
    # the chain: the recursions are not called until a frame exists
    sep = StreamSeparator(2, dereverb=True, beamform=True)
    for i in range(3):
        y = sep.process(x[:, 20 * i:20 * (i + 1)])
        assert y.shape == (1, 2, 0) and y.dtype == torch.int16
    assert sep.samples_seen == 60 and sep.samples_out == 0
    assert sep.dereverb.frames_seen == 0 and sep.separate.frames_seen == 0 and sep.beamform.frames_seen == 0
    y = sep.process(x[:, 60:260])                                        # 3 frames: one hop
    assert y.shape == (1, 2, 64) and sep.separate.frames_seen == 3 and sep.samples_out == 64


# ---- a captured graph -------------------------------------------------------------------------------------------------------------
def test_captured_graph_replayed_over_three_blocks():
    """one eager call of 256 samples (the tables exist, the stream is past its first 128 samples), then ONE captured
    process_into of 256 samples replayed over three blocks with fresh input copied in = the eager stream, bit for bit: from
    there on a launch depends on samples_seen through samples_seen mod 64 alone.  The same for the synthesis with 4 frames per
    call from frames_seen = 4.  (A single stream of launches: no parallel branches in the graph.)"""
    _need_gpu()
    from misonet_amd.stft import IstftStream, StftStream
    x, _ = _wave(2, 64 * 33 + 5, 8)
    eager = StftStream(8, 2)
    want = [eager.process(x[:, 256 * i:256 * (i + 1)]) for i in range(4)]
    X, _, _ = _spec(3, 66)
    ieager = IstftStream(3, int16=True)
    iwant = [ieager.process(X[:, 4 * i:4 * (i + 1)]) for i in range(4)]
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        st, ist = StftStream(8, 2), IstftStream(3, int16=True)
        assert _same(st.process(x[:, :256]), want[0]) and _same(ist.process(X[:, :4]), iwant[0])
        xb = torch.zeros((2, 256, 8), dtype=torch.float32, device="cuda")
        out = torch.empty((2, 8, st.frames(256), 129), dtype=torch.complex64, device="cuda")
        Xb = torch.zeros((3, 4, 129), dtype=torch.complex64, device="cuda")
        iout = torch.empty((3, 64 * ist.hops(4)), dtype=torch.int16, device="cuda")
        assert out.shape[2] == 4 and iout.shape[1] == 256
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            st.process_into(xb, out)
            ist.process_into(Xb, iout)
        for i in range(1, 4):
            xb.copy_(x[:, 256 * i:256 * (i + 1)])
            Xb.copy_(X[:, 4 * i:4 * (i + 1)])
            graph.replay()
            assert _same(out, want[i]) and _same(iout, iwant[i]), i
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()


# ---- the chain ------------------------------------------------------------------------------------------------------------------
CHAIN_L = 64 * 40 + 17


@functools.lru_cache(maxsize=None)
def _chain(M):
    """the padded recording [1, Lp, M] on the device and the rows of the existing one-shot path over all its frames: stft_hip ->
    DereverbStream -> SeparateStream(images=True) -> BeamformStream, and SeparateStream alone"""
    from misonet_amd import stft as S
    from misonet_amd.beamform import BeamformStream
    from misonet_amd.blind import SeparateStream
    from misonet_amd.dereverb import DereverbStream
    wav = np.ascontiguousarray(iva_ref.g8_sample()[0][4000:4000 + CHAIN_L, :M])
    sig = torch.nn.functional.pad(torch.from_numpy(wav).cuda(), (0, 0, 0, (-CHAIN_L) % 64))[None].contiguous()
    spec = S.stft_hip(sig)
    T = spec.shape[2]
    assert T == sig.shape[1] // 64 + 1 == 42
    d, s, b = DereverbStream(M, 129, 1, taps=3), SeparateStream(M, 129, 1), BeamformStream(M, M, 129, 1)
    der = d.process(spec)
    _est, img = s.process(der, images=True)
    full = S.istft_int16(b.process(img, der)[0].contiguous())                                    # [M, 64 (T - 1)]
    s2 = SeparateStream(M, 129, 1)
    plain = S.istft_int16(s2.process(spec)[0].contiguous())
    for st in (d, s, b, s2):
        assert not bool(st.fail.any())                                   # a condition on the input, not a tolerance
    assert full.shape == plain.shape == (M, 64 * (T - 1)) and int(full.abs().max()) > 100 and not _same(full, plain)
    return wav, sig, full, plain


def _run_chain(sep, sig, block):
    out = [sep.process(sig[:, a:a + block]) for a in range(0, sig.shape[1], block)] if block else []
    out.append(sep.flush() if block else sep.flush(sig))
    return torch.cat(out, dim=2)


@pytest.mark.parametrize("M", [2, 3])
def test_the_chain_equals_the_one_shot_path(M):
    _need_gpu()
    from misonet_amd.beamform import OnlineBeamformer
    from misonet_amd.dereverb import OnlineDereverb
    from misonet_amd.stream import StreamSeparator, separate_stream
    wav, sig, full, plain = _chain(M)
    sep = StreamSeparator(num_mic=M, dereverb=OnlineDereverb(taps=3), beamform=OnlineBeamformer())
    assert sep.latency_samples == 255
    for block in (64, 1000, 0):                                          # 0: the whole recording goes in with the flush
        got = _run_chain(sep.reset(), sig, block)
        assert got.dtype == torch.int16 and got.shape == (1, M, 64 * 41)
        assert (sep.samples_seen, sep.samples_out) == (sig.shape[1], 64 * 41)
        fail = sep.fail
        assert sorted(fail) == ["beamform", "dereverb", "separate"] and not any(bool(v.any()) for v in fail.values())
        for r in range(M):
            assert torch.equal(got[0, r], full[r]), (M, block, r)
    # the separation alone, and a choice of rows
    sep = StreamSeparator(num_mic=M, separate=True)
    for block in (64, 1000):
        assert _same(_run_chain(sep.reset(), sig, block)[0], plain), block
    assert sorted(sep.fail) == ["separate"] and not bool(sep.fail["separate"].any())
    one = StreamSeparator(num_mic=M, dereverb=OnlineDereverb(taps=3), beamform=OnlineBeamformer(), rows=[1])
    got = _run_chain(one, sig, 1000)
    assert got.shape == (1, 1, 64 * 41) and torch.equal(got[0, 0], full[1])
    # separate_stream: pads to whole hops, trims to L; ndarray in, ndarray out
    y = separate_stream(wav, block=1000, dereverb=OnlineDereverb(taps=3), beamform=OnlineBeamformer())
    assert isinstance(y, np.ndarray) and y.dtype == np.int16 and y.shape == (M, CHAIN_L)
    assert np.array_equal(y, full[:, :CHAIN_L].cpu().numpy())
    yt = separate_stream(torch.from_numpy(wav).cuda(), block=64, separate=True, rows=[1, 0])
    assert yt.is_cuda and _same(yt, plain[[1, 0], :CHAIN_L].contiguous())


def test_the_transforms_alone_pass_the_microphones_through():
    """separate=None: STFT -> iSTFT, float32; the stream's bits are those of istft(stft_hip(.)) of the whole recording"""
    _need_gpu()
    from misonet_amd import stft as S
    from misonet_amd.stream import StreamSeparator
    x, spec = _wave(1, 64 * 33, 2)
    sep = StreamSeparator(2, separate=None, int16=False)
    got = _run_chain(sep, x, 256)
    assert sep.fail == {} and got.dtype == torch.float32
    assert _same(got[0], S.istft(spec[0].contiguous()))


# ---- misuse -----------------------------------------------------------------------------------------------------------------------
def test_misuse_raises_before_any_launch():
    _need_gpu()
    from misonet_amd.stft import IstftStream, StftStream
    from misonet_amd.stream import StreamSeparator, separate_stream
    x, _ = _wave(1, 64 * 5 + 17, 2)
    X = _spec(3, 5)[0]
    st = StftStream(2)
    state0 = st.state.clone()
    for bad in (x.cpu(), x.double(), x[:, :, :1], x[0, :, 0], x.expand(2, -1, -1), np.zeros((64, 2), np.float32),
                torch.zeros((1, 0, 2), device="cuda")):
        with pytest.raises(ValueError):
            st.process(bad)
    with pytest.raises(ValueError):
        st.process_into(x[:, :256].contiguous(), torch.empty((1, 2, 2, 129), dtype=torch.complex64, device="cuda"))
    with pytest.raises(ValueError):
        st.process_into(x[:, :256].contiguous(), torch.empty((1, 2, 3, 129), dtype=torch.complex128, device="cuda"))
    assert st.samples_seen == 0 and torch.equal(st.state, state0)
    st.flush(x)
    for call in (lambda: st.process(x), lambda: st.flush(), lambda: st.flush(x)):
        with pytest.raises(ValueError):
            call()
    st.reset().process(x)
    ist = IstftStream(3)
    for bad in (X.cpu(), X.to(torch.complex128), X[:2], X[..., :128], torch.view_as_real(X), X[:, :0]):
        with pytest.raises(ValueError):
            ist.process(bad)
    with pytest.raises(ValueError):
        ist.process_into(X.contiguous(), torch.empty((3, 64 * 3), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        ist.process_into(X.contiguous(), torch.empty((3, 64 * 2), dtype=torch.float32, device="cuda"))
    assert ist.frames_seen == 0
    ist.flush(X)
    for call in (lambda: ist.process(X), lambda: ist.flush()):
        with pytest.raises(ValueError):
            call()
    for kw in (dict(num_mic=0), dict(num_mic=65), dict(num_mic=2, batch=0), dict(num_mic=2, batch=65536)):
        with pytest.raises(ValueError):
            StftStream(**kw)
    for rows in (0, 65536):
        with pytest.raises(ValueError):
            IstftStream(rows)
    for kw in (dict(rows=[2]), dict(rows=[]), dict(ref_ch=2), dict(separate=None, beamform=True), dict(separate="cauchy"),
               dict(dereverb=dict(taps=0))):
        with pytest.raises(ValueError):
            StreamSeparator(2, **kw)
    with pytest.raises(ValueError):
        StreamSeparator(9)                                               # the recursions take 2 .. 8 microphones
    with pytest.raises(ValueError):
        separate_stream(np.zeros((100,), np.float32))
    with pytest.raises(ValueError):
        separate_stream(np.zeros((100, 2), np.float32), block=0)
