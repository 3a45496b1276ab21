"""GPU tests of the streaming polyphase resampler (csrc/resample_stream.hip, ``misonet_amd.resample.ResampleStream``, the two ends
of ``misonet_amd.stream.StreamSeparator``).  No tolerance appears here: every comparison is exact equality, against the offline
kernel (``resample`` of the whole signal, whose float64 accuracy tests/test_gpu_resample.py holds) or against the uncut stream.

The main test runs, for each of the nine ratios and each of the four pairs of sample kinds, every (M, B, source layout) of
M in {1, 2, 6, 7, 8} x B in {1, 3} x {time-major, channel-major} over every length of ``resample_ref.lengths`` taken with the
stream's own tile; the cuttings (all at once, single samples, q, C - 1, C, C + 1, two seeded random sequences, each with the flush
carrying the last block or none) rotate through that grid three at a time, so that every (length, cutting) pair and every
(M, B, layout, length) is met for every ratio and kind without running their full product (the arithmetic of that rotation is
checked without a GPU, in tests/test_resample_stream.py).  Beyond that: more than 16 channels, buffers that held NaN, a NaN's
exact footprint across a call boundary, calls that emit nothing, reset, independence of the batch and reproducibility, a captured
graph with both resamplers replayed over three blocks, the ABI past 2^33 samples, the chain at 48 and 44.1 kHz against the offline
composition, and misuse."""
import functools
import itertools

import numpy as np
import pytest
import torch

import iva_ref
import resample_ref as R
import rstream_ref as S
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu

KINDS = [(False, False), (True, False), (False, True), (True, True)]          # (int16 in, int16 out)
NMAX = 2100


def _tile():
    from misonet_amd import _lib
    return int(_lib.lib().misonet_resample_stream_tile())


@functools.lru_cache(maxsize=None)
def _signal(i16, chan_major):
    """[3, NMAX, 8] on the device, time-major or (a transposed view of [3, 8, NMAX]) channel-major: made once, never written to"""
    x = np.stack([R.noise(NMAX, 8, 40 + b, dtype=np.int16 if i16 else np.float32) for b in range(3)])
    t = torch.from_numpy(x).cuda()
    return t.transpose(1, 2).contiguous().transpose(1, 2) if chan_major else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _cuttings(n, q, Cc, seed):
    rnd = [1, max(q - 1, 1), q, q + 1, max(Cc, 1), Cc + 1, 1000]
    r = np.random.default_rng(seed)
    base = [[n], [1], [q], [max(Cc - 1, 1)], [max(Cc, 1)], [Cc + 1], r.choice(rnd, 400).tolist(), r.choice(rnd, 400).tolist()]
    return [(c, wb) for c in base for wb in (True, False)]


def _run(st, x, pieces, with_block):
    """x [B, n, M] through the stream in blocks of ``pieces``, the flush with the last block or alone -> [B, n_out, M]"""
    st.reset()
    blocks, at, out = S.cut(x.shape[1], pieces), 0, []
    for k, b in enumerate(blocks):
        last = with_block and k == len(blocks) - 1
        want = st.outputs(b, last)
        y = st.flush(x[:, at:at + b]) if last else st.process(x[:, at:at + b])
        assert y.shape == (x.shape[0], want, x.shape[2])
        out.append(y)
        at += b
    if not with_block:
        out.append(st.flush())
    return torch.cat(out, dim=1)


# ---- the stream against the offline kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=lambda k: ("i16" if k[0] else "f32") + "-" + ("i16" if k[1] else "f32"))
@pytest.mark.parametrize("name", list(R.RATIOS))
def test_stream_equals_offline_bit_for_bit(name, kind):
    _need_gpu()
    from misonet_amd.resample import ResampleStream, resample
    fi, fo = R.RATIOS[name]
    p, q = R.pq(fi, fo)
    Cc = S.carry(p, q)
    lengths = R.lengths(p, q, _tile())
    assert lengths[-1] <= NMAX
    for li, (M, B, cm) in enumerate(itertools.product(R.CHANNELS, (1, 3), (False, True))):
        st = ResampleStream(M, fi, fo, batch=B, in_int16=kind[0], out_int16=kind[1])
        assert st.carry == Cc and st.latency == S.latency(p, q)
        for ni, n in enumerate(lengths):
            x = _signal(kind[0], cm)[:B, :n, :M]
            want = resample(x, fi, fo, out_int16=kind[1])
            assert want.shape == (B, R.out_len(n, p, q), M)
            cuts = _cuttings(n, q, Cc, n + M)
            for k in range(3):
                pieces, wb = cuts[(li + 3 * ni + 5 * k) % len(cuts)]
                got = _run(st, x, pieces, wb)
                assert _same(got, want.contiguous()), (M, B, cm, n, pieces[:8], wb)
                assert (st.samples_seen, st.samples_out) == (n, R.out_len(n, p, q))


@pytest.mark.parametrize("M", [17, 33])
def test_more_than_16_channels(M):
    _need_gpu()
    from misonet_amd.resample import ResampleStream, resample
    x = torch.from_numpy(np.stack([R.noise(700, M, 7 + b) for b in range(2)])).cuda()
    for fi, fo in ((48000, 16000), (16000, 44100)):
        want = resample(x, fi, fo)
        st = ResampleStream(M, fi, fo, batch=2)
        for pieces in ([700], [1, 61, 200, 3]):
            assert _same(_run(st, x, pieces, False), want), (M, fi, fo, pieces)


# ---- buffers that held NaN, and a NaN's footprint -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=str)
def test_buffers_that_held_nan(kind):
    """state and outputs pre-filled with NaN (int16: -12345): reset writes every byte of the state, a call every element of its
    output"""
    _need_gpu()
    from misonet_amd.resample import ResampleStream, resample
    fi, fo = R.RATIOS["160/441"]
    x = _signal(kind[0], False)[:, :700, :7]
    want = resample(x, fi, fo, out_int16=kind[1])
    st = ResampleStream(7, fi, fo, batch=3, in_int16=kind[0], out_int16=kind[1])
    st.state.view(torch.float32).fill_(float("nan"))
    st.reset()
    outs, at = [], 0
    for b, flush in [(20, False), (300, False), (1, False), (379, False), (0, True)]:
        shape = (3, st.outputs(b, flush), 7)
        out = torch.full(shape, -12345, dtype=torch.int16, device="cuda") if kind[1] else \
            torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
        st.process_into(x[:, at:at + b], out, flush)
        outs.append(out)
        at += b
    got = torch.cat(outs, dim=1)
    assert _same(got, want) and bool(torch.isfinite(got.float()).all())


@pytest.mark.parametrize("name", ["1/3", "3/1", "160/441", "147/160"])
def test_a_nan_reaches_exactly_its_support_across_a_call_boundary(name):
    _need_gpu()
    from misonet_amd.resample import ResampleStream
    fi, fo = R.RATIOS[name]
    p, q = R.pq(fi, fo)
    Cc, n = S.carry(p, q), 900
    x = _signal(False, False)[:1, :n, :2].clone()
    j = 400
    x[0, j, 1] = float("nan")
    st = ResampleStream(2, fi, fo)
    # the NaN is the last sample of a call, the first of a call, and C - 1 back in the carried tail when its last output comes
    for pieces in ([j + 1, 1000], [j, 1000], [j + 1, Cc - 1, 1, 1000], [1]):
        got = _run(st, x, pieces, False)[0]
        hit = torch.from_numpy(R.support(j, n, p, q)).cuda()
        assert bool(torch.isfinite(got[:, 0]).all()), pieces
        assert torch.equal(torch.isnan(got[:, 1]), hit) and int(hit.sum()) > 0, pieces


# ---- calls that emit nothing, reset, the batch --------------------------------------------------------------------------------
def test_calls_that_emit_nothing_still_advance_the_state():
    _need_gpu()
    from misonet_amd.resample import ResampleStream, resample
    fi, fo = R.RATIOS["1/3"]
    x = _signal(False, True)[:1, :500, :2]
    want = resample(x, fi, fo)
    st = ResampleStream(2, fi, fo)
    for i in range(3):                                                    # 30 samples: output 0 needs sample 30
        y = st.process(x[:, 10 * i:10 * (i + 1)])
        assert y.shape == (1, 0, 2) and y.dtype == torch.float32
    assert (st.samples_seen, st.samples_out) == (30, 0)
    y = st.process(x[:, 30:31])
    assert y.shape == (1, 1, 2) and _same(y, want[:, :1].contiguous())
    z = st.process(x[:, 31:33])                                           # 33 samples: output 1 needs sample 33
    assert z.shape == (1, 0, 2)
    rest = st.flush(x[:, 33:])
    assert _same(torch.cat([y, rest], dim=1), want.contiguous()) and st.samples_out == want.shape[1]
    with pytest.raises(ValueError):
        st.process(x[:, :10])                                             # spent until reset


def test_reset_batch_independence_and_run_to_run():
    _need_gpu()
    from misonet_amd.resample import ResampleStream
    fi, fo = R.RATIOS["147/160"]
    x = _signal(True, False)[:, :800, :6]
    pieces = [33, 1, 160, 21, 22, 300]
    st = ResampleStream(6, fi, fo, batch=3, in_int16=True)
    a = _run(st, x, pieces, True)
    st.reset().process(x[:, :100])                                        # a stream abandoned half-way, then reset
    b = _run(st, x, pieces, True)
    assert _same(a, b)
    assert _same(_run(ResampleStream(6, fi, fo, batch=3, in_int16=True), x, pieces, True), a)
    for i in range(3):
        one = ResampleStream(6, fi, fo, batch=1, in_int16=True)
        assert _same(_run(one, x[i:i + 1], pieces, True), a[i:i + 1]), i


# ---- a captured graph ----------------------------------------------------------------------------------------------------------
def test_captured_graph_with_both_resamplers_replayed_over_three_blocks():
    """The resampler in front of a chain (48 -> 16 kHz, float32, q = 3) and the one behind it (16 -> 44.1 kHz, int16 -> int16 on
    a channel-major view, q = 160).  One eager call puts each stream past its start (the taps exist, e > 0); then ONE captured
    pair of process_into with n_new = 4 q each, replayed over three blocks with fresh input copied in = the eager streams, bit for
    bit: a launch knows samples_seen only through the place of its first output against its block.  (A single stream of
    launches: no parallel branches in the graph.)"""
    _need_gpu()
    from misonet_amd.resample import ResampleStream
    xa = _signal(False, False)[:2, :, :6]
    xb = _signal(True, True)[:2, :, :3]
    fa, na, fb, nb = 120, 12, 100, 640

    def pair():
        return (ResampleStream(6, 48000, 16000, batch=2),
                ResampleStream(3, 16000, 44100, batch=2, in_int16=True, out_int16=True))

    ea, eb = pair()
    first = (ea.process(xa[:, :fa]), eb.process(xb[:, :fb]))
    assert first[0].shape[1] > 0 and first[1].shape[1] > 0
    want = [(ea.process(xa[:, fa + na * i:fa + na * (i + 1)]), eb.process(xb[:, fb + nb * i:fb + nb * (i + 1)]))
            for i in range(3)]
    assert want[0][0].shape == (2, 4, 6) and want[0][1].shape == (2, 4 * 441, 3)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ga, gb = pair()
        assert _same(ga.process(xa[:, :fa]), first[0]) and _same(gb.process(xb[:, :fb]), first[1])
        ba = torch.zeros((2, na, 6), dtype=torch.float32, device="cuda")
        bb = torch.zeros((2, 3, nb), dtype=torch.int16, device="cuda").transpose(1, 2)
        oa = torch.empty((2, ga.outputs(na), 6), dtype=torch.float32, device="cuda")
        ob = torch.empty((2, 3, gb.outputs(nb)), dtype=torch.int16, device="cuda").transpose(1, 2)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ga.process_into(ba, oa)
            gb.process_into(bb, ob)
        # the host's counters advanced once, at the capture; replays do not move them (process_into's docstring)
        assert (ga.samples_seen, gb.samples_seen) == (fa + na, fb + nb)
        for i in range(3):
            ba.copy_(xa[:, fa + na * i:fa + na * (i + 1)])
            bb.copy_(xb[:, fb + nb * i:fb + nb * (i + 1)])
            graph.replay()
            assert _same(oa, want[i][0]) and _same(ob.contiguous(), want[i][1].contiguous()), i
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()


# ---- the ABI past 2^33 samples --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1/3", "160/441", "441/160"])
def test_abi_at_n_seen_past_two_to_the_33(name):
    """n_seen = q 2^33, a zero state, a block of n samples: the call emits e(n_seen + n) - e(n_seen) outputs, and the last e(n) of
    them are a fresh stream's outputs for the same block (n_seen is a multiple of q: the same phase), bit for bit"""
    _need_gpu()
    from misonet_amd import _lib
    from misonet_amd.resample import ResampleStream
    lib = _lib.lib()
    fi, fo = R.RATIOS[name]
    p, q = R.pq(fi, fo)
    Cc, n, M, B = S.carry(p, q), 777, 3, 2
    x = _signal(False, False)[:B, :n, :M].contiguous()
    fresh = ResampleStream(M, fi, fo, batch=B).process(x)
    seen = q << 33
    cnt = int(lib.misonet_resample_stream_outputs(seen, n, 0, fi, fo))
    assert cnt == S.emitted(seen + n, p, q) - S.emitted(seen, p, q) and S.emitted(n, p, q) == fresh.shape[1] <= cnt
    state = torch.zeros(B * M * Cc, dtype=torch.float32, device="cuda")
    out = torch.full((B, cnt, M), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.misonet_resample_stream(x.data_ptr(), 0, x.stride(0), x.stride(2), x.stride(1), B, M, n, seen, 0, fi, fo,
                                           out.data_ptr(), 0, out.stride(0), out.stride(2), out.stride(1), state.data_ptr(),
                                           state.numel() * 4, _lib.stream_ptr(x.device)))
    assert bool(torch.isfinite(out).all()) and _same(out[:, cnt - fresh.shape[1]:].contiguous(), fresh)
    # the state after the call: the block's last C samples, per (item, channel)
    assert torch.equal(state.view(B, M, Cc), x[:, n - Cc:].transpose(1, 2))


# ---- the chain -------------------------------------------------------------------------------------------------------------------
CHAIN_HOPS = 40


@functools.lru_cache(maxsize=None)
def _recording(fs_in):
    """two microphones of the six-microphone recording, taken as a recording at fs_in that gives about 40 hops at 16 kHz"""
    L = (64 * CHAIN_HOPS + 17) * fs_in // 16000
    return np.ascontiguousarray(iva_ref.g8_sample()[0][4000:4000 + L, :2])


def _offline(wav, fs_in, fs_out, int16, **kw):
    """resample -> separate_stream at the model's rate -> resample, one after the other"""
    from misonet_amd.resample import resample
    from misonet_amd.stream import separate_stream
    mid = separate_stream(resample(wav, fs_in, 16000), block=1000, int16=int16, **kw)          # [R, L']
    rate = fs_in if fs_out == "in" else fs_out
    y = np.ascontiguousarray(resample(np.ascontiguousarray(mid.T), 16000, rate, out_int16=int16).T)
    if rate == fs_in and y.shape[1] != wav.shape[0]:                      # back at the input's rate: its length, as pcm_to_rate
        fit = np.zeros((y.shape[0], wav.shape[0]), dtype=y.dtype)
        fit[:, :min(wav.shape[0], y.shape[1])] = y[:, :wav.shape[0]]
        y = fit
    return y


@pytest.mark.parametrize("int16", [True, False])
@pytest.mark.parametrize("fs_in,fs_out", [(48000, "in"), (44100, 44100)])
def test_the_chain_at_another_rate_equals_the_offline_composition(fs_in, fs_out, int16):
    _need_gpu()
    from misonet_amd.stream import separate_stream
    wav = _recording(fs_in)
    p, q = R.pq(fs_in, 16000)
    want = _offline(wav, fs_in, fs_out, int16)
    assert want.shape == (2, wav.shape[0]) and want.dtype == (np.int16 if int16 else np.float32)
    assert float(np.abs(want.astype(np.float64)).max()) > (100 if int16 else 100 / 32767)
    for block in (-(-64 * q // p), 1000, wav.shape[0]):                   # 64 samples at the model's rate; 1000; the whole
        got = separate_stream(wav, block=block, fs=16000, fs_in=fs_in, fs_out=fs_out, int16=int16)
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and np.array_equal(got, want), (block,)
    got = separate_stream(torch.from_numpy(wav).cuda(), block=1000, fs=16000, fs_in=fs_in, fs_out=fs_out, int16=int16)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)


def test_the_chain_with_dereverberation_and_beamformer_at_48_khz():
    _need_gpu()
    from misonet_amd.beamform import OnlineBeamformer
    from misonet_amd.dereverb import OnlineDereverb
    from misonet_amd.stream import separate_stream
    wav = _recording(48000)
    kw = dict(dereverb=OnlineDereverb(taps=3), beamform=OnlineBeamformer())
    want = _offline(wav, 48000, "in", True, **kw)
    got = separate_stream(wav, block=192, fs=16000, fs_in=48000, fs_out="in", **kw)
    assert np.array_equal(got, want) and int(np.abs(want).max()) > 100


def test_one_resampler_only_latency_and_rateless_chain():
    _need_gpu()
    from misonet_amd.resample import resample
    from misonet_amd.stream import StreamSeparator, separate_stream
    wav = _recording(48000)
    x16 = resample(wav, 48000, 16000)
    mid = separate_stream(x16, block=1000)                                # int16 [2, L'] at the model's rate
    # fs_in only: the waves are at the model's rate
    sep = StreamSeparator(2, fs=16000, fs_in=48000)
    assert sep.resample_in is not None and sep.resample_out is None
    sig = torch.from_numpy(wav).cuda()[None]
    out = [sep.process(sig[:, a:a + 500]) for a in range(0, sig.shape[1], 500)] + [sep.flush(pad=True)]
    got = torch.cat(out, dim=2)[0]
    assert got.dtype == torch.int16 and np.array_equal(got.cpu().numpy(), mid)
    assert (sep.samples_seen, sep.samples_out) == (wav.shape[0], mid.shape[1])
    assert sep.latency_seconds == 30 / 48000 + 255 / 16000 and sep.latency_samples == 255
    # fs_out only: the blocks are at the model's rate
    sep = StreamSeparator(2, fs=16000, fs_out=44100)
    assert sep.resample_in is None and sep.resample_out is not None
    s16 = torch.from_numpy(x16).cuda()[None]
    out = [sep.process(s16[:, a:a + 64]) for a in range(0, s16.shape[1], 64)] + [sep.flush(pad=True)]
    got = torch.cat(out, dim=2)[0]
    want = np.ascontiguousarray(resample(np.ascontiguousarray(mid.T), 16000, 44100, out_int16=True).T)
    assert np.array_equal(got.cpu().numpy(), want) and sep.samples_out == want.shape[1]
    assert sep.latency_seconds == 255 / 16000 + (4410 / 441) / 16000
    both = StreamSeparator(2, fs=16000, fs_in=44100, fs_out="in")
    assert both.latency_seconds == (4410 / 160) / 44100 + 255 / 16000 + (4410 / 441) / 16000
    # a block that completes no sample at the model's rate skips the rest of the chain
    y = both.process(torch.from_numpy(_recording(44100)[:20]).cuda())
    assert y.shape == (1, 2, 0) and y.dtype == torch.int16 and both.stft.samples_seen == 0 and both.samples_seen == 20
    # fs alone, or rates that are the model's: not one link added
    for kw in (dict(fs=16000), dict(fs=16000, fs_in=16000, fs_out="in"), dict()):
        sep = StreamSeparator(2, **kw)
        assert sep.resample_in is None and sep.resample_out is None
    assert np.array_equal(separate_stream(x16, block=1000, fs=16000, fs_in=16000), mid)


# ---- misuse -----------------------------------------------------------------------------------------------------------------------
def test_misuse():
    _need_gpu()
    import misonet_amd
    from misonet_amd.resample import ResampleStream
    from misonet_amd.stream import StreamSeparator
    assert misonet_amd.ResampleStream is ResampleStream
    with pytest.raises(ValueError):
        StreamSeparator(2, fs_in=48000)                                   # rates without fs
    with pytest.raises(ValueError):
        StreamSeparator(2, fs_out="in")
    with pytest.raises(ValueError):
        StreamSeparator(2, fs=16000, fs_out="out")
    with pytest.raises(ValueError):
        StreamSeparator(2, fs=16000, fs_in=16001)                         # max(p, q) > 1024
    with pytest.raises(ValueError):
        StreamSeparator(2).latency_seconds
    with pytest.raises(ValueError):
        ResampleStream(2, 16001, 16000)
    with pytest.raises(ValueError):
        ResampleStream(0, 48000, 16000)
    st = ResampleStream(2, 48000, 16000, in_int16=True)
    f32 = torch.zeros((1, 90, 2), dtype=torch.float32, device="cuda")
    i16 = torch.zeros((1, 90, 2), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        st.process(f32)                                                   # a dtype that contradicts in_int16
    with pytest.raises(ValueError):
        st.process(i16[:, :, :1])
    with pytest.raises(ValueError):
        st.process(i16.cpu())
    assert st.outputs(90) == 20
    with pytest.raises(ValueError):
        st.process_into(i16, torch.zeros((1, 19, 2), dtype=torch.float32, device="cuda"))       # a wrong out shape
    with pytest.raises(ValueError):
        st.process_into(i16, torch.zeros((1, 20, 2), dtype=torch.int16, device="cuda"))         # ... and a wrong out dtype
    with pytest.raises(ValueError):
        st.outputs(0)
    # a time axis made by expand(): stride 0, 2 elements of storage behind 90 samples -- refused, nothing read
    with pytest.raises(ValueError):
        st.process(torch.zeros((1, 1, 2), dtype=torch.int16, device="cuda").expand(1, 90, 2))
    with pytest.raises(ValueError):
        st.process_into(i16, torch.zeros((1, 1, 2), dtype=torch.float32, device="cuda").expand(1, 20, 2))
    with pytest.raises(ValueError):
        st.process_into(i16, torch.zeros((1, 20, 1), dtype=torch.float32, device="cuda").expand(1, 20, 2))
    # ... while an expanded CHANNEL axis of the block is a legitimate view (the same samples for every channel), and a block of
    # one sample has no time stride to speak of
    assert st.samples_seen == 0 and st.process(i16[:, :, :1].expand(1, 90, 2)).shape == (1, 20, 2)
    st.reset()
    assert st.process(torch.zeros((1, 1, 2), dtype=torch.int16, device="cuda").expand(1, 1, 2)).shape == (1, 0, 2)
    st.reset()
    assert st.samples_seen == 0 and st.process(i16).shape == (1, 20, 2)
    st.flush()
    with pytest.raises(ValueError):
        st.flush()
