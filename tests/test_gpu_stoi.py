"""GPU tests of STOI / ESTOI (csrc/stoi.hip, misonet_amd/score.py): the resampled signals against SciPy within the bound of
their summation order, the kept frames and both figures against the explicit form of tests/stoi_ref.py on every test input
(real speech from tests/golden/g16_stoi.npz and synthetic AR(2) speech-like noise with gated pauses at 8, 10 and 16 kHz),
bit-reproducibility, independence of the batch and of the layout, the rules of the edges, and the recording paths with
``stoi=True``.

Measured on one MI355X: resampled signals within 7.4e-3 of their bound; largest deviation of STOI / ESTOI from the oracle over
the golden and the nine synthetic recordings (every pair, the mixture rows included) 1.9e-15, so the ceiling asserted is 1e-13
(ten times that, rounded up to a power of ten; the issue's condition is 1e-6).  The device is float64 and differs from NumPy
only in the order of its sums and the factorisation of the transform.  The module prints both figures (``[stoi] resampler
...``, ``[stoi] all inputs ...``)."""
import json
import os

import numpy as np
import pytest
import torch

import stoi_ref
from conftest import golden
from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

# The resampler: a sum of <= 117 products, each rounded once (2^-53) and added in sequence, so the device and SciPy are each
# within 118 x 2^-53 = 1.3e-14 of the exact sum, relative to sum_j |x[j] g[.]|; the taps of the two differ by <= 8.9e-16
# absolute (tests/test_stoi.py), which moves a sum by at most that x sum_j |x[j]| <= 117 max|x|.
RES_TOL = 4e-14
TAP_TOL = 2e-15
MARGIN_MIN = 1e-3     # dB: every compared input keeps its nearest frame this far from the 40 dB threshold (set by the issue)
DEV_CEIL = 1e-13      # STOI units against the explicit oracle: ten times the measured 1.9e-15, rounded up to a power of ten
                      # (the condition the issue sets on it: <= 1e-6)

# (fs, L, S, SNR of the added noise in dB, int16 estimates)
CASES = [(16000, 192000, 2, 5.0, True), (16000, 64000, 3, -5.0, False), (16000, 30011, 1, 20.0, False),
         (8000, 96000, 2, 20.0, False), (8000, 40000, 1, 5.0, True), (8000, 23456, 3, -5.0, True),
         (10000, 50000, 2, -5.0, True), (10000, 120000, 1, 20.0, False), (10000, 33000, 2, 5.0, False)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _golden_case():
    g = golden("g16_stoi.npz")
    est = (g["est_q"].astype(np.float64) / float(1 << 23)).astype(np.float32)            # 24-bit integers: exact in float32
    clean = g["clean"]
    return est, clean, (clean[0] + clean[1]).astype(np.float32), int(g["fs"]), g


def _synthetic(k):
    fs, L, S, snr, i16 = CASES[k]
    est, clean, mix = stoi_ref.case(k, S, L, fs, snr)
    return (stoi_ref.to_i16(est) if i16 else est), clean, mix, fs


@pytest.mark.parametrize("fs", stoi_ref.RATES)
@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
def test_resampled_signals_against_scipy(fs, i16):
    """B = 3 with different n_valid, contiguous and time-major views, lengths down to one sample"""
    _need_gpu()
    from misonet_amd import score
    worst = 0.0
    for n, E, R in ((1, 1, 1), (700, 2, 2), (5003, 4, 4), (40000, 2, 3)):
        rng = np.random.default_rng(n + fs)
        refs = np.stack([[stoi_ref.speechlike(7 * b + j, n, fs) if n > 100 else np.full(n, 0.3, np.float32)
                          for j in range(R)] for b in range(3)])
        est = (refs[:, np.arange(E) % R] + 0.02 * rng.standard_normal((3, E, n))).astype(np.float32)
        mix = refs.sum(axis=1, keepdims=True).astype(np.float32)
        if i16:
            est = stoi_ref.to_i16(est)
        nvs = [n, max(1, n - 100), max(1, (2 * n) // 3)]
        nv_dev = torch.tensor(nvs, dtype=torch.int32, device="cuda")
        d_r = _dev(refs.transpose(0, 2, 1)).transpose(1, 2)                 # time-major [B, n, R], read in place
        d_e_tm = _dev(est.transpose(0, 2, 1)).transpose(1, 2)
        for use_nv in (False, True):
            nv = nv_dev if use_nv else None
            x10, len10 = score.stoi_resample(_dev(est), d_r, _dev(mix), nv, fs)
            again = score.stoi_resample(_dev(est), d_r, _dev(mix), nv, fs)
            assert torch.equal(x10, again[0]) and torch.equal(len10, again[1])            # two calls: the same bits
            other = score.stoi_resample(d_e_tm, _dev(refs), _dev(mix), nv, fs)
            assert torch.equal(x10, other[0]) and torch.equal(len10, other[1])            # the layout moves no bit
            n10 = score.stoi_resampled_len(n, fs)
            assert tuple(x10.shape) == (3, R + E + 1, n10)
            got, lens = x10.cpu().numpy(), len10.cpu().numpy()
            for b in range(3):
                m = nvs[b] if use_nv else n
                assert lens[b] == score.stoi_resampled_len(m, fs) == -(-m * 10000 // fs)
                sigs = [refs[b, j] for j in range(R)] + [stoi_ref.as_f64(est[b, i]) for i in range(E)] + [mix[b, 0]]
                for s, x in enumerate(sigs):
                    x = np.asarray(x, dtype=np.float64)[:m]
                    want = stoi_ref.resample_scipy(x, fs)
                    _, mag, terms = stoi_ref.resample_sum(x, fs, return_abs=True)
                    assert want.shape[0] == lens[b]
                    lim = RES_TOL * mag + TAP_TOL * terms * np.abs(x).max()
                    err = np.abs(got[b, s, :lens[b]] - want)
                    assert np.all(err <= lim), (fs, n, b, s, float(err.max()), float(lim.min()))
                    assert not got[b, s, lens[b]:].any()                    # zero past the item's own length
                    worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
    print(f"[stoi] resampler fs={fs} {'int16' if i16 else 'float32'}: worst error / bound = {worst:.3e}")


_seen = {}


def _compare(tag, est, clean, mix, fs):
    """the device against the explicit oracle on one recording: returns the largest deviation in STOI / ESTOI units"""
    from misonet_amd import score
    want = stoi_ref.recording(est, clean, mix, fs)
    got = score.stoi_waves(est, clean, mix, fs=fs)
    margin = float(np.min(want["margin"]))
    assert margin >= MARGIN_MIN, (tag, want["margin"])                       # no frame can flip on a rounding difference
    assert list(got.frames) == list(want["frames"]) and list(got.frames_kept) == list(want["frames_kept"]), tag
    assert list(got.valid) == list(want["valid"]) and got.perm_best == want["perm_best"], tag
    assert got.fs == fs and got.n_samples == clean.shape[1]
    S = clean.shape[0]
    d = 0.0
    for key in ("stoi", "estoi", "stoi_best", "estoi_best", "stoi_mix", "estoi_mix", "stoi_i", "estoi_i"):
        d = max(d, float(np.abs(np.asarray(getattr(got, key)) - want[key]).max()))
    # every pair, crossed ones included: the block the dataclass is read from
    row = score.stoi_queue([(est, clean, mix)], fs, torch.device("cuda", torch.cuda.current_device()))[0].cpu().numpy()
    fig = row[:2 * S * (S + 1)].reshape(S + 1, S, 2)
    d = max(d, float(np.abs(fig[:S, :, 0] - want["stoi_matrix"]).max()), float(np.abs(fig[:S, :, 1] - want["estoi_matrix"]).max()))
    print(f"[stoi] {tag}: stoi {want['stoi']} estoi {want['estoi']} mix {want['stoi_mix']} kept {want['frames_kept']} of "
          f"{want['frames']}, margin {margin:.4f} dB: device - oracle {d:.3e}")
    return d


def test_golden_against_the_explicit_oracle():
    _need_gpu()
    from misonet_amd import score
    est, clean, mix, fs, g = _golden_case()
    d = _compare("golden", est, clean, mix, fs)
    got = score.stoi_waves(est, clean, mix, fs=fs)
    # the recorded figures of the oracle (the mixture there is the float64 sum; rounding it to float32 moves 1e-8)
    assert np.abs(got.stoi - np.diag(g["stoi"])).max() <= DEV_CEIL and np.abs(got.estoi - np.diag(g["estoi"])).max() <= DEV_CEIL
    assert np.abs(got.stoi_mix - g["stoi_mix"]).max() <= 1e-6 and list(got.frames_kept) == [427, 462]
    assert list(got.frames) == [624, 624]
    _seen["golden"] = d
    assert d <= DEV_CEIL, d


@pytest.mark.parametrize("k", range(len(CASES)))
def test_figures_against_the_explicit_oracle(k):
    _need_gpu()
    est, clean, mix, fs = _synthetic(k)
    d = _compare(f"case {k} {CASES[k]}", est, clean, mix, fs)
    _seen[k] = d
    assert d <= DEV_CEIL, (CASES[k], d)
    if len(_seen) == len(CASES) + 1:
        print(f"[stoi] all inputs: largest deviation from the oracle {max(_seen.values()):.3e} (ceiling {DEV_CEIL:.0e})")


def _block(est, refs, mix, nv, fs):
    from misonet_amd import score
    nv_dev = torch.tensor(nv, dtype=torch.int32, device="cuda") if nv is not None else None
    return score.stoi_block(_dev(est), _dev(refs), _dev(mix) if mix is not None else None, nv_dev, fs).cpu().numpy()


@pytest.mark.parametrize("fs", [8000, 16000])
def test_reproducible_and_independent_of_the_batch(fs):
    _need_gpu()
    from misonet_amd import score
    lens = (20000, 64000, 33333)
    S = 2
    items = [stoi_ref.case(20 + b, S, L, fs, 5.0) for b, L in enumerate(lens)]
    n = max(lens)
    est = np.zeros((3, S, n), np.int16)
    refs = np.zeros((3, S, n), np.float32)
    mix = np.zeros((3, 1, n), np.float32)
    junk = np.random.default_rng(1)
    for b, (e, r, m) in enumerate(items):
        est[b, :, :lens[b]], refs[b, :, :lens[b]], mix[b, 0, :lens[b]] = stoi_ref.to_i16(e), r, m
        est[b, :, lens[b]:] = 7777                                  # what lies past n_valid must not matter
        refs[b, :, lens[b]:] = junk.standard_normal((S, n - lens[b]))
        mix[b, 0, lens[b]:] = 1.0
    batch = _block(est, refs, mix, list(lens), fs)
    assert np.array_equal(batch, _block(est, refs, mix, list(lens), fs))                 # two calls: the same bits
    assert np.isfinite(batch).all() and batch.shape == (3, 2 * S * (S + 1) + 3 * S)
    # the layout moves no bit: time-major estimates and references
    tm = score.stoi_block(_dev(est.transpose(0, 2, 1)).transpose(1, 2), _dev(refs.transpose(0, 2, 1)).transpose(1, 2),
                          _dev(mix), torch.tensor(lens, dtype=torch.int32, device="cuda"), fs).cpu().numpy()
    assert np.array_equal(tm, batch)
    for b in range(3):
        e, r, m = items[b]
        alone = _block(stoi_ref.to_i16(e)[None], r[None], m[None, None], None, fs)
        assert np.array_equal(alone[0], batch[b]), b
        for pos in range(3):                                        # the same recording as item 0, 1, 2 of another batch
            order = [(b + k - pos) % 3 for k in range(3)]
            moved = _block(est[order], refs[order], mix[order], [lens[o] for o in order], fs)
            assert order[pos] == b and np.array_equal(moved[pos], batch[b]), (b, pos)
        one = score.stoi_waves(stoi_ref.to_i16(e), r, m, fs=fs)
        assert json.dumps(one.as_dict(), sort_keys=True) == json.dumps(
            score.stoi_unpack(batch[b], S, fs, lens[b]).as_dict(), sort_keys=True)
    # stoi_queue pads and batches by itself: the same rows
    q = score.stoi_queue([(stoi_ref.to_i16(e), r, m) for e, r, m in items], fs, torch.device("cuda", torch.cuda.current_device()))
    assert np.array_equal(q.cpu().numpy(), batch)


def test_short_silent_and_swapped():
    _need_gpu()
    from misonet_amd import score
    fs = 16000
    # below one frame, and fewer than 30 frames: 1e-5, not valid (pystoi's answer)
    for L, frames in ((200, 0), (6000, 28)):
        x = stoi_ref.speechlike(2, L, fs, pauses=False)[None]
        st = score.stoi_waves(x, x, x[0], fs=fs)
        assert list(st.frames) == [frames] and st.stoi[0] == 1e-5 and st.estoi[0] == 1e-5 and st.stoi_mix[0] == 1e-5
        assert list(st.valid) == [False] and st.n_samples == L
    # a signal against itself
    x = stoi_ref.speechlike(1, 3 * fs, fs)[None]
    st = score.stoi_waves(x, x, fs=fs)
    assert abs(st.stoi[0] - 1.0) <= 1e-12 and abs(st.estoi[0] - 1.0) <= 1e-12 and st.stoi_mix is None and st.stoi_i is None
    # a silent reference: NaN, not valid; the other speaker keeps its bits
    est, clean, mix = stoi_ref.case(4, 2, 3 * fs, fs, 5.0)
    full = score.stoi_waves(est, clean, mix, fs=fs)
    clean0 = clean.copy()
    clean0[1] = 0
    si = score.stoi_waves(est, clean0, mix, fs=fs)
    assert list(si.valid) == [True, False] and np.isnan(si.stoi[1]) and np.isnan(si.estoi[1]) and np.isnan(si.stoi_mix[1])
    assert si.stoi[0] == full.stoi[0] and si.estoi[0] == full.estoi[0] and si.perm_best == [0, 1]
    # swapped estimates
    sw = score.stoi_waves(est[::-1].copy(), clean, mix, fs=fs)
    assert full.perm_best == [0, 1] and sw.perm_best == [1, 0]
    assert np.array_equal(sw.stoi_best, full.stoi) and np.array_equal(sw.estoi_best, full.estoi)
    assert np.array_equal(sw.stoi_mix, full.stoi_mix) and np.all(sw.stoi < full.stoi - 0.3)
    # host or device inputs, arrays or tensors: the same answer
    again = score.stoi_waves(torch.from_numpy(est), torch.from_numpy(clean).cuda(), mix, fs=fs)
    assert json.dumps(again.as_dict(), sort_keys=True) == json.dumps(full.as_dict(), sort_keys=True)
    with pytest.raises(ValueError):
        score.stoi_waves(est, clean[:1], fs=fs)
    with pytest.raises(ValueError):
        score.stoi_waves(est, clean, mix[:-1], fs=fs)
    with pytest.raises(ValueError, match="8000, 10000 or 16000"):
        score.stoi_waves(est, clean, mix, fs=44100)


def _same(a, b):
    return json.dumps(a.as_dict(), sort_keys=True) == json.dumps(b.as_dict(), sort_keys=True)      # bit for bit


def test_recording_with_stoi(nets):
    import misonet_amd as mz
    from misonet_amd import score
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    L = 100000
    obs, s0, s1 = synthetic_utterance(40, L)
    refs = np.stack([s0[:, 0], s1[:, 0]])
    pcm0, sc0 = enh.enhance_recording(obs, [s0, s1], max_batch=16, score=True)
    pcm, sc, st = enh.enhance_recording(obs, [s0, s1], max_batch=16, score=True, stoi=True)
    assert np.array_equal(pcm, pcm0) and _same(sc, sc0)                                  # stoi moves no bit of pcm or Score
    assert _same(st, score.stoi_waves(pcm, refs, obs[:, 0], fs=16000)) and st.n_samples == L and st.fs == 16000
    print(f"[stoi] recording: stoi {st.stoi} estoi {st.estoi} mix {st.stoi_mix} kept {st.frames_kept} of {st.frames}")
    _, _, ev0 = enh.enhance_recording(obs, [s0, s1], score=True, bss=True, bss_filt_len=64)
    p4, s4, ev, st4 = enh.enhance_recording(obs, [s0, s1], score=True, bss=True, bss_filt_len=64, stoi=True)
    assert np.array_equal(p4, pcm0) and _same(s4, sc0) and _same(ev, ev0) and _same(st4, st)
    st8 = enh.enhance_recording(obs, [s0, s1], score=True, stoi=True, fs=8000)[2]        # the figure at the call's fs
    assert _same(st8, score.stoi_waves(pcm, refs, obs[:, 0], fs=8000)) and st8.fs == 8000
    others = [synthetic_utterance(41 + i, n) for i, n in enumerate((70000, 64000, 130001))]
    recs = [(o[0], [o[1], o[2]], f"x{i}") for i, o in enumerate(others)]
    recs.insert(2, (obs, [s0, s1], "me"))
    plain = enh.enhance_recordings(recs, max_batch=4, score=True)
    with_bss = enh.enhance_recordings(recs, max_batch=4, score=True, bss=True, bss_filt_len=64)
    seen = []
    for mb in (4, 16):
        out = enh.enhance_recordings(recs, max_batch=mb, score=True, stoi=True)
        assert list(out) == ["x0", "x1", "me", "x2"]
        for name, (o, c, _) in zip(out, recs):
            p, s, t = out[name]
            assert np.array_equal(p, plain[name][0]) and _same(s, plain[name][1])
            assert _same(t, score.stoi_waves(p, np.stack([c[0][:, 0], c[1][:, 0]]), o[:, 0], fs=16000)), name
        assert _same(out["me"][2], st)
        seen.append(out)
    assert all(_same(seen[0][k][2], seen[1][k][2]) for k in seen[0])
    both = enh.enhance_recordings(recs, max_batch=4, score=True, bss=True, bss_filt_len=64, stoi=True)
    for name in both:
        p, s, e, t = both[name]
        assert np.array_equal(p, plain[name][0]) and _same(s, plain[name][1]) and _same(e, with_bss[name][2])
        assert _same(t, seen[0][name][2])
    with pytest.raises(ValueError):
        enh.enhance_recording(obs, [s0, s1], stoi=True)
    with pytest.raises(ValueError):
        enh.enhance_recordings(recs, stoi=True)
    with pytest.raises(ValueError):
        enh.enhance_recording(obs, None, score=True, stoi=True)
    with pytest.raises(ValueError, match="8000, 10000 or 16000"):
        enh.enhance_recording(obs, [s0, s1], score=True, stoi=True, fs=44100)


def test_score_eval_command_line_with_stoi(tmp_path):
    _need_gpu()
    import sys
    from misonet_amd import score, stft as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import score_eval
    est_dir, ref_dir = tmp_path / "est", tmp_path / "ref"
    est_dir.mkdir()
    ref_dir.mkdir()
    want, plain = {}, {}
    f = lambda q: ((q.astype(np.int32) << 8) / float(1 << 23)).astype(np.float32)   # noqa: E731  (what a wav reader returns)
    fs = 8000
    for k, (name, L) in enumerate((("u1", 30000), ("u2", 20000))):
        e, c, m = stoi_ref.case(30 + k, 2, L, fs, 5.0)
        cq = np.stack([stoi_ref.to_i16(c)] * 3, axis=2)                                  # [2, L, 3 channels]
        cq[:, :, 0] //= 2
        eq, mq = stoi_ref.to_i16(e), np.stack([stoi_ref.to_i16(m)] * 3, axis=1)
        for s in range(2):
            S.write_wav_pcm24(str(est_dir / f"{name}_{s}.wav"), eq[s], fs)
            S.write_wav_pcm24(str(ref_dir / f"{name}_{s}.wav"), cq[s], fs)
        S.write_wav_pcm24(str(ref_dir / f"{name}.wav"), mq, fs)
        want[name] = score.stoi_waves(eq, f(cq[:, :, 1]), f(mq[:, 1]), fs=fs).as_dict()
        plain[name] = score.score_waves(eq, f(cq[:, :, 1]), f(mq[:, 1])).as_dict()
    out, out0 = tmp_path / "stoi.json", tmp_path / "plain.json"
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "1", "--out", str(out), "--stoi"])
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "1", "--out", str(out0)])
    with open(out) as fh:
        doc = json.load(fh)
    with open(out0) as fh:
        doc0 = json.load(fh)
    assert sorted(doc) == ["mean", "u1", "u2"]
    for name in want:
        assert doc[name]["stoi"] == want[name] and doc[name]["stoi"]["fs"] == fs and doc[name]["stoi"]["perm_best"] == [0, 1]
        assert {k: v for k, v in doc[name].items() if k != "stoi"} == plain[name] == doc0[name]    # without the flag: unchanged
    assert "stoi" not in doc0["mean"] and {k: v for k, v in doc["mean"].items() if k != "stoi"} == doc0["mean"]
    vals = [v for n in want for v in want[n]["stoi"]]
    assert abs(doc["mean"]["stoi"]["stoi"] - np.mean(vals)) <= 1e-12 and doc["mean"]["stoi"]["n_speakers_valid"] == 4
