"""GPU tests of SRMR (csrc/srmr.hip, misonet_amd/score.py): the mean modulation energies, the figure, the 90 % bandwidth, K*, the
frames and the validity against form (a) of tests/srmr_ref.py (scipy.signal.lfilter + scipy.signal.hilbert) at the frame edges
(both rates), at the seams of the chunked scan, around one LDS pass of the transform (P = 4096 | 8192 | 16384), on one long input
(600 000 samples, P = 2^20), on a synthetic family (dry and three T60s, both rates, int16 and float32, 1 .. 3 signals with a
mixture) and on the real speech of tests/golden/g16_stoi.npz; bit-reproducibility, independence of the batch, of the position in
it and of the layout, untouched pads and scratch; int16 against float32; the recording paths with ``srmr=True``; graph capture.

Measured on one MI355X over all these inputs: the largest deviation device - oracle (a) is 3.1e-12 (the 4 Hz band of one channel of
the 8192-sample input; 9e-14 on the long one), with d64 = 1.0e-12 .. 2.3e-12 between the two forms of the oracle beside it: a change
of the envelope by one unit in its last place moves form (a) itself by 1.4e-12, because the 4 Hz modulation filter in direct form
has its poles next to z = 1, so no realisation on the device can come closer to form (a) than that.  The ceiling asserted is
1e-10 (ten times the largest deviation, rounded up to a power of ten); the smallest shift of a planted fault is 1.45e-8
(tests/test_srmr.py), 145 times the ceiling.  The module prints the deviation of every input (``[srmr] <input>: ...``).

int16 against float32: float32(q / 32767) is not the value an int16 sample stands for, and form (a) itself moves by 9e-9 between the
two; the test feeds q / 32768, which float32 holds exactly, and accounts for the known gain 32767 / 32768 (the energies scale by
its square, everything else is invariant)."""
import json
import os

import numpy as np
import pytest
import torch

import srmr_ref as sr
from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

DEV_CEIL = sr.DEV_CEIL
WORST = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _result(out, cnt, en, b, s):
    v = float(out[b, s, 0])
    return dict(energy=en[b, s].cpu().numpy(), srmr=v, k_star=int(out[b, s, 1]), bw=float(out[b, s, 2]), frames=int(cnt[b, s]),
                valid=bool(np.isfinite(v)))


def _check(tag, got, want, fs):
    if not want["valid"]:
        assert not got["valid"] and np.isnan(got["srmr"]) and np.isnan(got["bw"]) and got["k_star"] == 0, tag
        assert got["frames"] == want["frames"] and (want["frames"] > 0 or np.isnan(got["energy"]).all()), tag
        print(f"[srmr] {tag}: invalid, frames {got['frames']}")
        return
    assert sr.margin_ok(want, fs), (tag, want["run"], want["bw"])
    assert got["valid"] and got["k_star"] == want["k_star"] and got["frames"] == want["frames"], (tag, got, want["k_star"])
    d = sr.deviation(want, got)
    WORST[tag] = d
    print(f"[srmr] {tag}: srmr {want['srmr']:.6f} K* {want['k_star']} BW {want['bw']:.2f} frames {want['frames']}; "
          f"device - oracle {d:.2e} (ceiling {DEV_CEIL:.0e})")
    assert d <= DEV_CEIL, (tag, d)


def _measure_one(x, fs):
    from misonet_amd import score
    out, cnt, en = score.srmr_measure(_dev(x)[None, None], fs=fs, energy=True)
    return _result(out, cnt, en, 0, 0)


@pytest.mark.parametrize("fs", sr.RATES)
def test_edge_lengths_against_the_oracle(fs):
    """frames 0 | 1 | 1 | 2; at 16 kHz also C - 1, C, C + 1, 2 C + 1, 3 C and 4096, 4097, 8192, 8193 samples"""
    _need_gpu()
    from misonet_amd import score
    C = score.srmr_chunk()
    cases = sr.edge_lengths(fs, C)
    assert len(cases) >= (8 if fs == 16000 else 4)          # C = N_w at 16 kHz: C - 1, C, C + 1 are frame edges too
    for n, t60 in cases:
        _check(f"fs {fs} n {n} T60 {t60}", _measure_one(sr.signal(fs, n, t60), fs), sr.oracle_of(fs, n, t60), fs)
    x = sr.signal(fs, 9000, 0.7)
    print(f"[srmr] d64 (form a - form b) on 6000 samples at {fs} Hz: {sr.d64(x[:6000], fs):.2e}")


@pytest.mark.parametrize("k", range(len(sr.FAMILY)))
def test_family_against_the_oracle(k):
    """dry and three T60s, int16 and float32, 1 .. 3 signals and the mixture in one call, then the dataclass"""
    _need_gpu()
    from misonet_amd import score
    fs, n, t60s, tmix, i16 = sr.FAMILY[k]
    sig = np.stack([sr.signal(fs, n, t, i16) for t in t60s])
    mix = sr.mix_of(fs, n, tmix) if tmix is not None else None
    out, cnt, en = score.srmr_measure(_dev(sig)[None], _dev(mix)[None, None] if mix is not None else None, fs=fs, energy=True)
    for s, t in enumerate(t60s):
        _check(f"family {k} fs {fs} n {n} T60 {t} int16 {i16}", _result(out, cnt, en, 0, s), sr.oracle_of(fs, n, t, i16), fs)
    if mix is not None:
        _check(f"family {k} mixture T60 {tmix}", _result(out, cnt, en, 0, len(t60s)), sr.oracle_of(fs, n, tmix, False), fs)
    v = score.srmr_waves(sig, mix, fs=fs)
    o = out.cpu().numpy()[0]
    S = len(t60s)
    assert np.array_equal(v.srmr, o[:S, 0]) and list(v.k_star) == [int(x) for x in o[:S, 1]] and np.array_equal(v.bw90, o[:S, 2])
    assert list(v.frames) == [sr.frames_of(n, fs)] * S and all(v.valid) and v.fs == fs and v.n_samples == n
    if mix is not None:
        assert v.srmr_mix == o[S, 0] and np.array_equal(v.srmr_i, o[:S, 0] - o[S, 0])
        assert v.srmr_i[0] > 0                                          # the driest signal against the T60 = 1.2 s mixture
    else:
        assert v.srmr_mix is None and v.srmr_i is None


def test_long_input_against_the_oracle():
    """600 000 samples: P = 2^20 = 1024 x 1024, 147 chunks, 582 frames"""
    _need_gpu()
    fs, n, t60 = sr.LONG
    _check(f"long fs {fs} n {n}", _measure_one(sr.signal(fs, n, t60), fs), sr.oracle_of(fs, n, t60), fs)


def test_real_speech_against_the_oracle():
    _need_gpu()
    from misonet_amd import score
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_stoi.npz"))
    est, mix, fs = sr.golden_signals(g)
    lo, hi = sr.GOLDEN_SLICE
    est, mix = np.ascontiguousarray(est[:, lo:hi]), np.ascontiguousarray(mix[lo:hi])
    out, cnt, en = score.srmr_measure(_dev(est)[None], _dev(mix)[None, None], fs=fs, energy=True)
    for s, x in enumerate((est[0], est[1], mix)):
        _check(f"golden signal {s}", _result(out, cnt, en, 0, s), sr.measure(x, fs), fs)


def test_reproducible_and_independent_of_batch_layout_pad_and_scratch():
    _need_gpu()
    from misonet_amd import score
    fs, n, S = 16000, 20011, 2
    C = score.srmr_chunk()
    me = np.stack([sr.signal(fs, n, 0.3, True), sr.signal(fs, n, 1.2, True)])
    mix = sr.mix_of(fs, n, 1.2)
    alone = score.srmr_measure(_dev(me)[None], _dev(mix)[None, None], fs=fs, energy=True)
    again = score.srmr_measure(_dev(me)[None], _dev(mix)[None, None], fs=fs, energy=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(alone, again))                         # two runs
    # a batch of 5 with unequal n_valid, the recording first and last; the pad holds the int16 minimum / NaN: never read
    lens = [n, 2 * C + 1, 30000, 4095, n]
    nmax = max(lens)
    bsig = np.full((5, S, nmax), -32768, np.int16)
    bmix = np.full((5, 1, nmax), np.nan, np.float32)
    for b, L in enumerate(lens):
        bsig[b, :, :L] = me[:, :L] if L <= n else np.stack([sr.signal(fs, L, 0.3, True), sr.signal(fs, L, 0.7, True)])
        bmix[b, 0, :L] = mix[:L] if L <= n else sr.mix_of(fs, L, 1.2)
    nv = torch.tensor(lens, dtype=torch.int32).cuda()
    nb = score.srmr_scratch_bytes(5, S + 1, nmax, fs)
    scratch = torch.full((nb // 8,), float("nan"), dtype=torch.float64, device="cuda").view(torch.uint8)
    bat = score.srmr_measure(_dev(bsig), _dev(bmix), nv, fs=fs, energy=True, scratch=scratch)
    for b in (0, 4):
        assert all(torch.equal(x[b], y[0]) for x, y in zip(bat, alone)), b
    assert int(bat[1][3, 0]) == 0 and torch.isnan(bat[0][3, :, 0]).all()                # the item shorter than a frame
    assert not torch.isnan(bat[0][[0, 1, 2, 4]]).any() and not torch.isnan(bat[2][[0, 1, 2, 4]]).any()
    one = score.srmr_measure(_dev(bsig[1:2, :, :lens[1]]), _dev(bmix[1:2, :, :lens[1]]), fs=fs, energy=True)
    assert all(torch.equal(x[1], y[0]) for x, y in zip(bat, one))                       # an item with its own P and chunk count
    # time-major views of [n, S] and [n, 1] arrays, read in place
    tsig = _dev(np.ascontiguousarray(me.T))[None].transpose(1, 2)
    tmix = _dev(np.stack([mix, mix], axis=1))[None][:, :, :1].transpose(1, 2)
    assert tsig.stride(2) == S and tmix.stride(2) == 2
    tm = score.srmr_measure(tsig, tmix, fs=fs, energy=True)
    assert all(torch.equal(a, b) for a, b in zip(tm, alone))
    # the same through the queue of recordings of unequal length
    rows = score.srmr_queue([(me, mix), (bsig[2, :, :30000], bmix[2, 0, :30000])], fs, torch.device("cuda", 0)).cpu().numpy()
    v = score.srmr_unpack(rows[0], S, fs, n)
    assert np.array_equal(v.srmr, alone[0][0, :S, 0].cpu().numpy()) and v.srmr_mix == float(alone[0][0, S, 0])
    blocks = score.side_queue([(me, np.zeros((S, n), np.float32) + 0.01 * mix, mix)], torch.device("cuda", 0), srmr_fs=fs)
    assert len(blocks) == 4 and blocks[0] is None and blocks[1] is None and blocks[2] is None
    assert np.array_equal(blocks[3].cpu().numpy()[0], rows[0])


def test_int16_against_float32():
    """the float32 array q / 32768 holds exactly 32767 / 32768 times what the int16 array q stands for"""
    _need_gpu()
    fs, n = 16000, 20011
    q = sr.signal(fs, n, 0.3, True)
    a = _measure_one(q, fs)
    b = _measure_one((q.astype(np.float64) / 32768.0).astype(np.float32), fs)
    g2 = (32767.0 / 32768.0) ** 2
    b = dict(b, energy=b["energy"] / g2)
    d = sr.deviation(a, b)
    print(f"[srmr] int16 against float32: {d:.2e}")
    assert d <= DEV_CEIL, d


def test_graph_capture():
    _need_gpu()
    from misonet_amd import score
    fs, n = 8000, 14001
    sig, mix = _dev(np.stack([sr.signal(fs, n, 0.7), sr.signal(fs, n, 0.0)]))[None], _dev(sr.mix_of(fs, n, 1.2))[None, None]
    eager = score.srmr_measure(sig, mix, fs=fs, energy=True)                             # also builds the table
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                            # captures on a side stream
        held = score.srmr_measure(sig, mix, fs=fs, energy=True)
    for t in held:
        t.fill_(0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(held, eager))


def _same(a, b):
    return json.dumps(a.as_dict(), sort_keys=True) == json.dumps(b.as_dict(), sort_keys=True)      # bit for bit


def _recording(seed, L, mics=6):
    r = np.random.default_rng(seed)
    return sum((0.05 * r.standard_normal((L, mics))).astype(np.float32) for _ in range(2))


def test_recording_paths_with_srmr(nets):
    import misonet_amd as mz
    from misonet_amd import score
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    W, fs = 3072, 8000
    L = 2 * W + 100                                                                      # three windows at hop W / 2 ... W
    rec = _recording(51, L)
    plain, P0 = enh.enhance_continuous(rec, window=W, hop=W - 256, return_perms=True)
    assert P0.shape[0] == 3
    got, P, v = enh.enhance_continuous(rec, window=W, hop=W - 256, return_perms=True, fs=fs, srmr=True)
    assert np.array_equal(got, plain) and np.array_equal(P, P0)
    assert isinstance(v, score.Srmr) and _same(v, score.srmr_waves(got, rec[:, 0], fs=fs)) and v.n_samples == L and v.fs == fs
    assert v.frames[0] == sr.frames_of(L, fs) >= 1 and v.srmr_mix is not None
    got2, v2 = enh.enhance_continuous(rec, window=W, hop=W - 256, fs=fs, srmr=True, max_batch=1)
    assert np.array_equal(got2, plain) and _same(v2, v)
    print(f"[srmr] continuous: srmr {v.srmr} mix {v.srmr_mix} K* {v.k_star}")
    # enhance_recording without score and without clean sources
    base = enh.enhance_recording(rec, None, chunk_size=W)
    pcm, r = enh.enhance_recording(rec, None, chunk_size=W, fs=fs, srmr=True)
    assert np.array_equal(pcm, base) and _same(r, score.srmr_waves(pcm, rec[:, 0], fs=fs))
    short = enh.enhance_recording(rec[:1500], None, chunk_size=W, fs=fs, srmr=True)[1]   # shorter than a frame: invalid
    assert list(short.valid) == [False, False] and short.frames[0] == 0 and np.isnan(short.srmr).all()
    many = enh.enhance_recordings([(rec, None, "a"), (rec[:5000], None, "b")], chunk_size=W, fs=fs, srmr=True)
    assert np.array_equal(many["a"][0], base) and _same(many["a"][1], r)
    assert _same(many["b"][1], score.srmr_waves(many["b"][0], rec[:5000, 0], fs=fs))
    with pytest.raises(ValueError, match="8000 or 16000"):
        enh.enhance_recording(rec, None, chunk_size=W, fs=10000, srmr=True)
    # dereverb_wav: output channel ref_ch against input channel ref_ch
    wav = np.stack([sr.signal(fs, 9000, 0.7), sr.signal(fs, 9000, 1.2)], axis=1)
    y0 = mz.dereverb_wav(wav, fs)
    y, d = mz.dereverb_wav(wav, fs, srmr=True, ref_ch=1)
    assert np.array_equal(y, y0) and _same(d, score.srmr_waves(y[None, :, 1], wav[:, 1], fs=fs)) and d.valid[0]
    assert d.srmr_i is not None and len(d.srmr) == 1


def test_command_line_tools_with_srmr(tmp_path):
    _need_gpu()
    import sys
    from misonet_amd import score, stft as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import score_eval
    import srmr_eval
    est_dir, ref_dir = tmp_path / "est", tmp_path / "ref"
    est_dir.mkdir()
    ref_dir.mkdir()
    f = lambda q: ((q.astype(np.int32) << 8) / float(1 << 23)).astype(np.float32)   # noqa: E731  (what a wav reader returns)
    fs, want = 8000, {}
    for name, L in (("u1", 14001), ("u2", 9000)):
        eq = np.stack([sr.signal(fs, L, 0.0, True), sr.signal(fs, L, 0.7, True)])
        cq = np.stack([sr.signal(fs, L, 0.0, True), sr.signal(fs, L, 0.3, True)])
        mq = np.stack([sr.signal(fs, L, 1.2, True)] * 2, axis=1)                         # [L, 2 channels]
        for s in range(2):
            S.write_wav_pcm24(str(est_dir / f"{name}_{s}.wav"), eq[s], fs)
            S.write_wav_pcm24(str(ref_dir / f"{name}_{s}.wav"), cq[s], fs)
        S.write_wav_pcm24(str(ref_dir / f"{name}.wav"), mq, fs)
        want[name] = score.srmr_waves(eq, f(mq[:, 1]), fs=fs).as_dict()
    out, out0, out1 = tmp_path / "with.json", tmp_path / "plain.json", tmp_path / "srmr.json"
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "0", "--out", str(out), "--srmr"])
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "0", "--out", str(out0)])
    srmr_eval.main([str(est_dir), "--mix", str(ref_dir), "--ref-ch", "1", "--out", str(out1)])
    doc, doc0, doc1 = (json.load(open(p)) for p in (out, out0, out1))
    assert sorted(doc) == sorted(doc1) == ["mean", "u1", "u2"]
    for name in want:
        assert doc[name]["srmr"] == want[name] == doc1[name] and doc1[name]["fs"] == fs
        assert {k: v for k, v in doc[name].items() if k != "srmr"} == doc0[name]          # without the flag: unchanged
    assert "srmr" not in doc0["mean"] and {k: v for k, v in doc["mean"].items() if k != "srmr"} == doc0["mean"]
    assert doc["mean"]["srmr"] == doc1["mean"] and doc1["mean"]["n_signals_valid"] == 4
    vals = [v for n in want for v in want[n]["srmr"]]
    assert abs(doc1["mean"]["srmr"] - np.mean(vals)) <= 1e-12
