"""GPU tests of the polyphase resampler (csrc/resample.hip, ``misonet_amd.resample``) against
``scipy.signal.resample_poly`` in float64: nine ratios, the lengths of ``resample_ref.lengths`` (1, 2, shorter than the filter,
every residue class that matters, the tile edges of the kernel), 1 / 2 / 6 / 7 / 8 channels, both layouts, a strided view, int16
in and out, a batch with three lengths; impulses against the tap table; reproducibility, independence of the batch, buffers full of
NaN, a planted NaN, a captured HIP graph, the exact copy, strided views whose offsets pass 2^31; and the recording paths on the six-microphone sample of tests/golden.

Bar (``resample_ref.within_bar``): with e0 the rel-L2 of float32(ref64) against ref64, the float32 result is within 2 e0 of ref64
over the whole tensor and over the worst channel.  Every figure is printed (``[resample] ...``); LAB.md has them."""
import functools
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from test_gpu_parity import _need_gpu

pytestmark = pytest.mark.gpu
NAMES = list(R.RATIOS)


def _tile():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return int(_lib.lib().misonet_resample_tile())


TILE = _tile()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _dev(x, fs, **kw):
    """ndarray -> the device's result as an ndarray, through a device tensor"""
    from misonet_amd import resample as RS
    return RS.resample(torch.from_numpy(np.array(x)).cuda(), fs[0], fs[1], **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name, n, M, seed=0, int16=False):
    """(input, resample_poly of it in float64), computed once and left unchanged"""
    p, q = R.pq(*R.RATIOS[name])
    x = R.noise(n, M, seed=1000 * seed + 17 * n + M, dtype=np.int16 if int16 else np.float32)
    ref = R.oracle(x, p, q)
    if int16:
        ref = ref * (1.0 / 32767.0)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@pytest.mark.parametrize("name", NAMES)
def test_against_resample_poly(name):
    """every length x every channel count of one ratio against the bar; the figures of the worst case are printed"""
    _need_gpu()
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    worst = (-1.0, None)
    ns = R.lengths(p, q, TILE)
    for n in ns:
        for M in R.CHANNELS:
            x, ref = _case(name, n, M)
            y = _dev(x, fs)
            assert y.dtype == np.float32 and y.shape == ref.shape == (R.out_len(n, p, q), M), (n, M)
            ok, w, c, ew, ec = R.within_bar(y, ref)
            assert ok, (name, n, M, w, c, ew, ec)
            ratio = w / ew if ew > 0 else 0.0                 # 1 / 1 is exact: e0 = 0 and so is the error
            if ratio > worst[0]:
                worst = (ratio, (n, M, w, c, ew, ec))
    n, M, w, c, ew, ec = worst[1]
    print(f"[resample] {name}: n in {ns} x M in {list(R.CHANNELS)}: worst rel-L2 / e0 = {worst[0]:.3f} at n {n} M {M} "
          f"(whole {w:.3e}, channel {c:.3e}; e0 {ew:.3e}, {ec:.3e})")


@pytest.mark.parametrize("name", ["1/2", "3/1", "160/441", "147/160"])
def test_layouts_views_kinds_and_batches(name):
    """channel-major [M, L] in and out, every second microphone of [L, 12], int16 input, ndarray and CPU tensor round trips, and
    B = 3 with three lengths: each against the bar, and against the bits of the plain time-major call"""
    _need_gpu()
    from misonet_amd import resample as RS
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    n, M = max(1, -(-(TILE + 1) * q // p)), 6
    x, ref = _case(name, n, M)
    plain = _dev(x, fs)
    # channel-major: a transposed view of [M, L]; the result is channel-major in memory too
    cm = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    y = RS.resample(cm.t(), fs[0], fs[1])
    assert tuple(y.shape) == plain.shape and y.stride(0) == 1 and y.stride(1) == plain.shape[0]
    assert _same(y.cpu().numpy(), plain)
    # every second microphone of [L, 12], read in place
    wide = np.zeros((n, 12), np.float32)
    wide[:, ::2] = x
    wide[:, 1::2] = 7.0
    wd = torch.from_numpy(wide).cuda()
    view = wd[:, ::2]
    assert not view.is_contiguous()
    assert _same(RS.resample(view, fs[0], fs[1]).cpu().numpy(), plain)
    # ndarray in -> ndarray out, CPU tensor in -> CPU tensor out, [L] in -> [L] out
    a = RS.resample(np.array(x), fs[0], fs[1])
    assert isinstance(a, np.ndarray) and _same(a, plain)
    t = RS.resample(torch.from_numpy(np.array(x)), fs[0], fs[1])
    assert isinstance(t, torch.Tensor) and t.device.type == "cpu" and _same(t.numpy(), plain)
    one = RS.resample(np.ascontiguousarray(x[:, 2]), fs[0], fs[1])
    assert one.shape == (plain.shape[0],) and _same(one, np.ascontiguousarray(plain[:, 2]))
    # int16 input: q stands for q / 32767
    xi, refi = _case(name, n, M, int16=True)
    yi = _dev(xi, fs)
    ok, w, c, ew, ec = R.within_bar(yi, refi)
    print(f"[resample] {name} int16 in, n {n} M {M}: whole {w:.3e} channel {c:.3e} (e0 {ew:.3e}, {ec:.3e})")
    assert ok
    # B = 3, three lengths: each item is its own prefix resampled, then zeros
    nv = [n, max(1, n // 3), 1]
    xb = np.stack([R.noise(n, M, seed=40 + b) for b in range(3)])
    yb = _dev(xb, fs, n_valid=nv)
    assert yb.shape == (3,) + plain.shape
    for b in range(3):
        k = R.out_len(nv[b], p, q)
        refb = R.oracle(xb[b, :nv[b]], p, q)
        ok, w, c, ew, ec = R.within_bar(yb[b, :k], refb)
        assert ok, (b, w, c, ew, ec)
        assert not yb[b, k:].any()
        assert _same(yb[b, :k], _dev(xb[b, :nv[b]], fs))                    # ... with the bits of the prefix alone


@pytest.mark.parametrize("name", NAMES)
def test_impulses_give_the_table(name):
    """a unit impulse at each input position j mod q -- q consecutive positions, every residue, so that every entry of the
    table is met -- and at the first and the last sample, as the items of one launch (q + 2 of them at most): the float32 rounding of
    the table entries exactly, and exact zeros everywhere else"""
    _need_gpu()
    from misonet_amd import resample as RS
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    Lh = R.half_len(p, q)
    g = RS.taps(*fs)
    n = 2 * (Lh // p + 1) + 2 * q + 3
    mid = n // 2
    spots = sorted({0, n - 1} | {mid - q // 2 + r for r in range(q)})
    x = np.zeros((len(spots), n, 1), np.float32)
    for b, j in enumerate(spots):
        x[b, j, 0] = 1.0
    y = _dev(x, fs)
    m = np.arange(R.out_len(n, p, q), dtype=np.int64)
    met = np.zeros(g.size, dtype=bool)
    for b, j in enumerate(spots):
        t = m * q - j * p + Lh
        live = (t >= 0) & (t <= 2 * Lh)
        want = np.where(live, g[np.where(live, t, 0)], 0.0).astype(np.float32)
        assert np.array_equal(y[b, :, 0], want), (name, j)
        assert not y[b, ~live, 0].any()
        if 0 < j < n - 1:
            met[t[live]] = True
    assert met.all(), (name, int((~met).sum()))                     # the interior impulses alone meet every entry of the table
    print(f"[resample] {name}: impulses at {len(spots)} positions of n {n} give float32(g) exactly, all {g.size} entries met")


@pytest.mark.parametrize("name", ["1/1", "1/2", "2/1", "160/441", "441/160"])
def test_int16_output(name):
    """int16 out: within 1 LSB of rint(float64 x 32767) everywhere, equal to it wherever the float64 value is further than 1e-6
    from a half-integer (fewer than 0.1 % of the samples are nearer: noise puts about 2e-6 of them there), and saturated at
    -32768 / 32767"""
    _need_gpu()
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    n, M = max(2, -(-(2 * TILE + 1) * q // p)), 6
    for int16 in (False, True):
        x, ref = _case(name, n, M, seed=3, int16=int16)
        got = _dev(x, fs, out_int16=True).astype(np.int64)
        want, clear = R.rint_i16(ref)
        inside = 1.0 - clear.mean()
        print(f"[resample] {name} int16 out ({'int16' if int16 else 'float32'} in): {clear.size} samples, {inside:.2e} of them "
              f"within 1e-6 of a half-integer, max |diff| {int(np.abs(got - want).max())} LSB")
        assert inside <= 1e-3
        assert np.abs(got - want).max() <= 1 and np.array_equal(got[clear], want[clear])
    loud = (np.array(_case(name, n, M, seed=3)[0]) * 40.0).astype(np.float32)          # far past full scale: both limits
    got = _dev(loud, fs, out_int16=True).astype(np.int64)
    want, clear = R.rint_i16(R.oracle(loud, p, q))
    assert got.min() == -32768 and got.max() == 32767 and (got == 32767).sum() > 10 and (got == -32768).sum() > 10
    assert np.abs(got - want).max() <= 1 and np.array_equal(got[clear], want[clear])


def test_copy_is_exact():
    """1 / 1: float32 -> float32 is a copy bit for bit (NaN, infinities and denormals included); int16 -> float32 is the int16
    rule, q (1 / 32767) in float64 rounded once; int16 -> int16 gives the samples back"""
    _need_gpu()
    x = np.array(_case("1/1", 3 * TILE + 5, 7)[0])
    x[5, 2], x[9, 0], x[11, 6], x[13, 1] = np.nan, np.inf, -np.inf, 1e-42
    y = _dev(x, (8000, 8000))
    assert _same(y, x) and _same(_dev(x, (44100, 44100)), x)
    q = R.noise(700, 2, seed=5, dtype=np.int16)
    q[0, 0], q[1, 0] = -32768, 32767
    assert _same(_dev(q, (8000, 8000)), (q.astype(np.float64) * (1.0 / 32767.0)).astype(np.float32))
    back = _dev(q, (8000, 8000), out_int16=True)
    assert back.dtype == np.int16 and np.array_equal(back[1:], q[1:]) and back[0, 0] == -32768


@pytest.mark.parametrize("name", ["1/3", "441/160", "80/441"])
def test_reproducible_batch_independent_and_fully_written(name):
    """two runs: the same bits; every item alone: the bits it has inside the batch; a destination full of NaN comes back
    without one, float32 and int16"""
    _need_gpu()
    from misonet_amd import resample as RS
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    n, M, B = max(3, -(-(2 * TILE + 1) * q // p)), 7, 3
    xb = np.stack([R.noise(n, M, seed=60 + b) for b in range(B)])
    nv = [n, n - 1, max(1, n // 2)]
    a, b2 = _dev(xb, fs, n_valid=nv), _dev(xb, fs, n_valid=nv)
    assert _same(a, b2)
    for b in range(B):
        alone = _dev(xb[b:b + 1], fs, n_valid=nv[b:b + 1])
        assert _same(alone[0], a[b]), b
    src = torch.from_numpy(xb).cuda()
    nvd = torch.tensor(nv, dtype=torch.int32).cuda()
    n_out = R.out_len(n, p, q)
    dst = torch.full((B, n_out, M), float("nan"), dtype=torch.float32, device="cuda")
    RS.resample_into(src, dst, nvd, fs[0], fs[1])
    assert _same(dst.cpu().numpy(), a)
    d16 = torch.full((B, n_out, M), -12345, dtype=torch.int16, device="cuda")
    RS.resample_into(src, d16, nvd, fs[0], fs[1])
    assert _same(d16.cpu().numpy(), _dev(xb, fs, n_valid=nv, out_int16=True))
    assert not (d16.cpu().numpy() == -12345).all(axis=(1, 2)).any()


@pytest.mark.parametrize("name", ["1/2", "3/1", "160/441"])
def test_a_nan_reaches_its_support_and_nothing_else(name):
    """one NaN (and, in another channel, one infinity) in the input: non-finite exactly at the outputs of that channel whose taps
    cover the sample -- what the restatement gives -- and every other sample keeps its bits"""
    _need_gpu()
    fs = R.RATIOS[name]
    p, q = R.pq(*fs)
    n, M = max(3, -(-(TILE + 40) * q // p)), 6
    x = np.array(_case(name, n, M)[0])
    clean = _dev(x, fs)
    j_nan, j_inf = n // 2 + 1, n - 1
    x[j_nan, 4] = np.nan
    x[j_inf, 1] = np.inf
    y = _dev(x, fs)
    bad = ~np.isfinite(y)
    want = ~np.isfinite(R.restate(x, p, q))
    mask = np.zeros_like(bad)
    mask[:, 4] = R.support(j_nan, n, p, q)
    mask[:, 1] = R.support(j_inf, n, p, q)
    assert np.array_equal(want, mask)                                           # the restatement is the definition's support
    assert np.array_equal(bad, mask), (int(bad.sum()), int(mask.sum()))
    assert np.array_equal(_bits(y)[~mask], _bits(clean)[~mask])
    print(f"[resample] {name}: a NaN at sample {j_nan} reaches {int(mask[:, 4].sum())} outputs of its channel, "
          f"an infinity at the last sample {int(mask[:, 1].sum())}")


def test_hip_graph():
    """the call captured once the taps exist, replayed with new inputs copied in: the bits of the eager call"""
    _need_gpu()
    from misonet_amd import resample as RS
    fs = R.RATIOS["160/441"]
    p, q = R.pq(*fs)
    n, M, B = 1500, 6, 2
    inputs = [np.stack([R.noise(n, M, seed=80 + 10 * i + b) for b in range(B)]) for i in range(3)]
    eager = [_dev(x, fs) for x in inputs]                                       # the first of them builds the table
    assert not _same(eager[1], eager[2])
    src = torch.from_numpy(inputs[0]).cuda()
    dst = torch.zeros((B, R.out_len(n, p, q), M), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            RS.resample_into(src, dst, None, fs[0], fs[1])
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        src.copy_(torch.from_numpy(inputs[i]))
        dst.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert _same(dst.cpu().numpy(), eager[i]), i


# ---- the recording paths ------------------------------------------------------------------------------------------------------
def test_separate_recording_at_another_rate(tmp_path):
    """the six-microphone sample (8 kHz) up-sampled to 16 kHz with SciPy on the host, then separated with fs=8000, fs_in=16000:
    the bits of the run on resample()'s own output fed at 8 kHz; SI-SDR improvement within 0.1 dB of the restatement of
    tests/iva_ref.py on the SciPy-down-sampled input; with fs_out="in" the input's length and 16000 in the file header"""
    _need_gpu()
    import wave
    import iva_ref
    import misonet_amd as mz
    from misonet_amd import resample as RS, score as SC
    from scipy.signal import resample_poly
    wav8, clean, fs = iva_ref.g8_sample()
    wav16 = resample_poly(wav8.astype(np.float64), 2, 1, axis=0).astype(np.float32)             # [64000, 6]
    sep = mz.BlindSeparator(2, 6, ref_ch=0)
    pcm = sep.separate_recording(wav16, fs=fs, fs_in=16000, beamform=False)
    dev8 = RS.resample(wav16, 16000, fs)
    assert dev8.shape == wav8.shape
    assert np.array_equal(pcm, sep.separate_recording(dev8, fs=fs, beamform=False))
    assert pcm.dtype == np.int16 and pcm.shape == (2, wav8.shape[0])
    sc = SC.score_waves(pcm, clean, dev8[:, 0], fs=fs)
    got = float(np.mean(sc.si_sdr_best - sc.si_sdr_mix))
    host8 = resample_poly(wav16.astype(np.float64), 1, 2, axis=0)
    ok, w, c, ew, ec = R.within_bar(dev8, host8)
    assert ok
    r = iva_ref.auxiva_item(iva_ref.stft(host8.astype(np.float32)), 2)
    est = np.stack([iva_ref.istft(r["images"][s, :, 0, :], host8.shape[0]) for s in range(2)])
    _, want = iva_ref.si_sdr_improvement(est, clean.astype(np.float64), host8[:, 0])
    print(f"[resample] g8 sample 16 -> 8 kHz: rel-L2 vs resample_poly {w:.3e} (e0 {ew:.3e}); AuxIVA SI-SDR improvement "
          f"{got:.2f} dB (restatement on SciPy's input {want:.2f} dB)")
    assert abs(got - want) <= 0.1, (got, want)
    path = str(tmp_path / "out" / "g16")
    back = sep.separate_recording(wav16, fs=fs, fs_in=16000, fs_out="in", save_path=path, beamform=False)
    assert back.dtype == np.int16 and back.shape == (2, wav16.shape[0])
    up = RS.resample(np.ascontiguousarray(pcm.T), fs, 16000, out_int16=True).T
    assert np.array_equal(back, up[:, :wav16.shape[0]])
    for s in range(2):
        with wave.open(f"{path}_{s}.wav", "rb") as f:
            assert f.getframerate() == 16000 and f.getnframes() == wav16.shape[0] and f.getsampwidth() == 3
    x16, rate = RS.load_wav(f"{path}_0.wav")
    assert rate == 16000 and np.array_equal(x16[:, 0], (back[0].astype(np.float64) / 32768.0).astype(np.float32))
    x8, rate8 = RS.load_wav(f"{path}_0.wav", sr=8000)                       # the reference's loader line
    assert rate8 == 8000 and _same(x8, RS.resample(x16, 16000, 8000))
    with pytest.raises(ValueError):
        sep.separate_recording(wav16, fs=fs, fs_in=16001)


def test_enhance_recording_rates(sd1, sd3, tmp_path):
    """fs_in=None, fs_out=None is the call without them, bit for bit (the parent's path); fs_in with scores resamples the
    observation and the clean sources together and equals the call on resample()'s outputs; the other recording paths likewise"""
    _need_gpu()
    import misonet_amd as mz
    from misonet_amd import resample as RS, weights as W
    m1 = mz.MISO_1(2, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m1.load_state_dict(sd1)
    m3 = mz.MISO_3(1, 6, 7, list(W.DEFAULT_EN_CH), list(W.DEFAULT_DE_CH), "IN").cuda(0)
    m3.load_state_dict(sd3)
    enh = mz.Enhancer(m1.eval(), m3.eval(), num_spks=2, ref_ch=0)
    L, chunk = 9000, 4096
    obs, s0, s1 = W.synthetic_utterance(70, L)
    kw = dict(chunk_size=chunk, max_batch=2, fs=16000)
    plain = enh.enhance_recording(obs, [s0, s1], **kw)
    assert np.array_equal(plain, enh.enhance_recording(obs, [s0, s1], fs_in=None, fs_out=None, **kw))
    assert np.array_equal(plain, enh.enhance_recording(obs, [s0, s1], fs_in=16000, fs_out="in", **kw))   # nothing to do
    # a 48 kHz recording with scores: observation and clean sources go to 16 kHz in one launch
    up = [RS.resample(np.asarray(w, np.float32), 16000, 48000) for w in (obs, s0, s1)]
    down = [RS.resample(w, 48000, 16000) for w in up]
    got, sc = enh.enhance_recording(up[0], up[1:], fs_in=48000, score=True, **kw)
    want, sc0 = enh.enhance_recording(down[0], down[1:], score=True, **kw)
    assert np.array_equal(got, want) and got.shape == (2, L) and sc.as_dict() == sc0.as_dict()
    path = str(tmp_path / "rec")
    out48 = enh.enhance_recording(up[0], None, fs_in=48000, fs_out=48000, save_path=path, **kw)
    assert out48.dtype == np.int16 and out48.shape == (2, up[0].shape[0])
    assert RS.load_wav(path + "_1.wav")[1] == 48000
    base = enh.enhance_recording(down[0], None, **kw)
    assert np.array_equal(out48, RS.resample(np.ascontiguousarray(base.T), 16000, 48000, out_int16=True).T[:, :out48.shape[1]])
    many = enh.enhance_recordings([(up[0], None, "a"), (up[0][:20000], None, "b")], fs_in=48000, fs_out="in", **kw)
    assert np.array_equal(many["a"], out48) and many["b"].shape == (2, 20000)
    cont = enh.enhance_continuous(up[0], window=4096, fs=16000, fs_in=48000)
    assert np.array_equal(cont, enh.enhance_continuous(down[0], window=4096, fs=16000))
    d48 = mz.dereverb_wav(up[0], fs=16000, fs_in=48000, fs_out="in")
    assert isinstance(d48, np.ndarray) and d48.dtype == np.float32 and d48.shape == up[0].shape
    d16 = mz.dereverb_wav(down[0], fs=16000)
    assert _same(d48, RS.resample(d16, 16000, 48000)[:d48.shape[0]])
    assert _same(mz.dereverb_wav(down[0], fs=16000, fs_in=None, fs_out=None), d16)


def test_offsets_past_two_to_the_31():
    """every index is 64-bit: two int16 source samples 2^31 + 2 elements apart, then four int16 output samples whose last lies
    2^31 + 3 elements into its buffer, give the bits of the contiguous call.  An element offset past 2^31 needs a buffer of 2^31
    elements (4.3 GB of int16), whatever the shape: one such buffer at a time, allocated but not filled -- only the strided
    samples are touched -- and handed back to the driver at the end."""
    _need_gpu()
    from misonet_amd import resample as RS
    fs = R.RATIOS["2/1"]
    n, M = 2, 2
    x = np.array([[12000, -7000], [-30000, 25000]], dtype=np.int16)
    plain = _dev(x, fs, out_int16=True)                                         # [4, 2]
    n_out = plain.shape[0]
    assert n_out == 4 and plain.any(axis=1).all()
    xd = torch.from_numpy(x).cuda()[None]
    s_step = (1 << 31) + 2
    buf = torch.empty((n - 1) * s_step + M, dtype=torch.int16, device="cuda")
    src = torch.as_strided(buf, (1, n, M), (0, s_step, 1))
    src.copy_(xd)
    dst = torch.full((1, n_out, M), -1, dtype=torch.int16, device="cuda")
    RS.resample_into(src, dst, None, fs[0], fs[1])
    assert _same(dst[0].cpu().numpy(), plain)
    del src, buf
    torch.cuda.empty_cache()
    d_step = (1 << 31) // (n_out - 1) + 2
    assert (n_out - 1) * d_step > 1 << 31
    buf = torch.empty((n_out - 1) * d_step + M, dtype=torch.int16, device="cuda")
    dst = torch.as_strided(buf, (1, n_out, M), (0, d_step, 1))
    dst.fill_(-1)
    RS.resample_into(xd, dst, None, fs[0], fs[1])
    assert _same(dst[0].cpu().numpy(), plain)
    del dst, buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("M", [17, 20])
def test_more_than_sixteen_channels(M):
    """the Python call takes a wider input in groups of 16 channels, one launch each, through slices of the source and of the
    destination: time-major and channel-major in and out, against the bar and against the bits of every channel resampled alone"""
    _need_gpu()
    from misonet_amd import resample as RS
    name = "160/441"
    fs = R.RATIOS[name]
    x, ref = _case(name, 709, M, seed=7)
    y = _dev(x, fs)
    ok, w, c, ew, ec = R.within_bar(y, ref)
    print(f"[resample] {name} M {M} (groups of 16): whole {w:.3e} channel {c:.3e} (e0 {ew:.3e}, {ec:.3e})")
    assert ok and y.shape == ref.shape
    for ch in range(M):
        assert _same(np.ascontiguousarray(y[:, ch]), _dev(np.ascontiguousarray(x[:, ch]), fs)), ch
    cm = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()                     # [M, L]
    z = RS.resample(cm.t(), fs[0], fs[1])
    assert z.stride(0) == 1 and z.stride(1) == y.shape[0] and _same(z.cpu().numpy(), y)
    zi = RS.resample(cm.t(), fs[0], fs[1], out_int16=True)
    assert zi.stride(0) == 1 and _same(zi.cpu().numpy(), _dev(x, fs, out_int16=True))
