"""GPU tests of the scores (csrc/score.hip, misonet_amd/score.py): the device sums against the NumPy restatement
(tests/score_ref.py) within the worst-case bound of any summation order, bit-reproducible and independent of the batch; dB
values; the spectral criterion against criterion.py's own answers (tests/golden/g15_score.npz); score_waves on a known
answer; and the recording, loader and tester paths with ``score=True``."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import score_ref
from conftest import golden
from test_gpu_parity import nets, _need_gpu      # noqa: F401

pytestmark = pytest.mark.gpu

NS = (64, 4095, 4096, 4097, 64000, 191936)
DB_TOL = 1e-4      # dB: n 2^-53 = 2e-11 relative on the sums at n = 191936, x Cee / noise <= 1e6 at 60 dB, x 4.34 dB = 9e-5


def _layout(x, layout):
    """x host [B, C, n] -> a device view [B, C, n] with the values of x in the memory layout asked for"""
    B, C, n = x.shape
    t = torch.from_numpy(x).cuda()
    if layout == "contig":                                  # [B, C, n]: what istft_k writes
        return t.contiguous()
    if layout == "time_major":                              # [B, n, C]: clean_wav
        return t.transpose(1, 2).contiguous().transpose(1, 2)
    wide = torch.zeros((B, n, C + 3), dtype=t.dtype, device="cuda")      # [B, n, M] at channels 2..: the observation
    wide[:, :, 2:2 + C] = t.transpose(1, 2)
    return wide[:, :, 2:2 + C].transpose(1, 2)


def _signals(rng, B, E, R, n, i16):
    ref = (0.05 * rng.standard_normal((B, R, n))).astype(np.float32) + np.float32(0.01)
    est = (0.05 * rng.standard_normal((B, E, n))).astype(np.float32)
    est[:, : min(E, R)] += np.float32(0.5) * ref[:, : min(E, R)]
    if i16:
        est = (est * 32767.0).astype(np.int16)
    return est, ref


def _bound(est, ref, nv):
    """n 2^-52 sum |terms| for each of the 5 sums of every pair: [E, R, 5]"""
    c = score_ref.C16 if est.dtype == np.int16 else 1.0
    e = np.abs(est[:, :nv].astype(np.float64)) * c
    r = np.abs(ref[:, :nv].astype(np.float64))
    E, R = e.shape[0], r.shape[0]
    out = np.zeros((E, R, 5))
    out[..., 0] = e.sum(1)[:, None]
    out[..., 1] = r.sum(1)[None, :]
    out[..., 2] = (e * e).sum(1)[:, None]
    out[..., 3] = (r * r).sum(1)[None, :]
    out[..., 4] = e @ r.T
    return max(nv, 1) * 2.0 ** -52 * out


@pytest.mark.parametrize("layout", ["contig", "time_major", "mic"])
@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("E,R", [(1, 1), (3, 2), (4, 3), (5, 4)])
def test_wave_stats_against_numpy(E, R, i16, layout):
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(100 * E + 10 * R + int(i16))
    worst = 0.0
    for n in NS:
        est, ref = _signals(rng, 3, E, R, n, i16)
        big_e, big_r = _signals(rng, 16, E, R, n, i16)
        big_nv = [int(v) for v in rng.integers(1, n + 1, size=16)]
        for use_nv in (False, True):
            nvs = [n, max(1, n - 100), (2 * n) // 3] if use_nv else [n, n, n]
            d_e, d_r = _layout(est, layout), _layout(ref, layout)
            nv_dev = torch.tensor(nvs, dtype=torch.int32, device="cuda") if use_nv else None
            got_t = score.wave_stats(d_e, d_r, nv_dev)
            again = score.wave_stats(d_e, d_r, nv_dev)
            assert torch.equal(got_t, again), (n, use_nv)                     # two calls: the same bits
            got = got_t.cpu().numpy()
            assert got.shape == (3, E, R, 5) and got.dtype == np.float64
            for b in range(3):
                want = score_ref.wave_stats(est[b], ref[b], nvs[b])
                lim = _bound(est[b], ref[b], nvs[b])
                err = np.abs(got[b] - want)
                assert np.all(err <= lim), (n, use_nv, b, float((err / np.maximum(lim, 1e-300)).max()))
                worst = max(worst, float((err / np.maximum(lim, 1e-300)).max()))
            # the same items inside B = 16, at other positions, and alone (B = 1): bit-equal
            pos = [5, 0, 15]
            for b, q in enumerate(pos):
                big_e[q], big_r[q], big_nv[q] = est[b], ref[b], nvs[b]
            big = score.wave_stats(_layout(big_e, layout), _layout(big_r, layout),
                                   torch.tensor(big_nv, dtype=torch.int32, device="cuda") if use_nv else None).cpu().numpy()
            for b, q in enumerate(pos):
                assert np.array_equal(big[q], got[b]), (n, use_nv, b)
            one = score.wave_stats(_layout(est[1:2], layout), _layout(ref[1:2], layout),
                                   torch.tensor(nvs[1:2], dtype=torch.int32, device="cuda") if use_nv else None).cpu().numpy()
            assert np.array_equal(one[0], got[1]), (n, use_nv)
    print(f"[score] wave_stats E={E} R={R} {'int16' if i16 else 'float32'} {layout}: worst error / bound = {worst:.3e}")


def test_wave_stats_layouts_agree_bitwise():
    """a lane adds its samples in sample order whichever way they were loaded: the three layouts give the same bits"""
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(7)
    for i16 in (True, False):
        est, ref = _signals(rng, 2, 3, 2, 70001, i16)
        got = [score.wave_stats(_layout(est, lay), _layout(ref, lay)).cpu().numpy() for lay in ("contig", "time_major", "mic")]
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def _at_db(rng, n, db):
    """float32 r and e with SI-SDR(e, r) close to db"""
    r = rng.standard_normal(n)
    d = rng.standard_normal(n)
    rc, d = r - r.mean(), d - d.mean()
    d -= rc * (d @ rc) / (rc @ rc)
    d *= np.sqrt(0.49 * (rc @ rc) / 10.0 ** (db / 10.0) / (d @ d))
    return (0.05 * r).astype(np.float32), (0.05 * (0.7 * r + d)).astype(np.float32)


@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("n", [64000, 191936])
def test_db_values_from_device_statistics(n, i16):
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(n + int(i16))
    for db in (-20.0, 0.0, 20.0, 40.0, 60.0):
        r, e = _at_db(rng, n, db)
        est = (e * 32767.0).astype(np.int16) if i16 else e
        st = score.wave_stats(torch.from_numpy(est[None, None]).cuda(), torch.from_numpy(r[None, None]).cuda())[0].cpu().numpy()
        want_sdr, want_snr = score_ref.si_sdr_one(score_ref.wave_stats(est[None], r[None])[0, 0], n), \
            score_ref.snr_one(score_ref.wave_stats(est[None], r[None])[0, 0], n)
        got_sdr, got_snr = float(score.si_sdr(st, n)[0, 0]), float(score.snr(st, n)[0, 0])
        print(f"[score] n={n} {'int16' if i16 else 'float32'} target {db:+.0f} dB: SI-SDR ref {want_sdr:.9f} "
              f"device {got_sdr:.9f} (diff {abs(got_sdr - want_sdr):.2e}), SNR diff {abs(got_snr - want_snr):.2e}")
        assert -21.0 <= want_sdr <= 60.5
        assert abs(got_sdr - want_sdr) <= DB_TOL and abs(got_snr - want_snr) <= DB_TOL


@pytest.mark.parametrize("S", [2, 3])
def test_spec_pairs_against_the_reference_criterion(S):
    """the device against criterion.py's own loss_uPIT / loss_Enhance (the fixture holds their answers)"""
    _need_gpu()
    from misonet_amd import score
    g = golden("g15_score.npz")
    est, ref = torch.from_numpy(g[f"est{S}"]).cuda(), torch.from_numpy(g[f"ref{S}"]).cuda()
    pair, perm, val = score.spec_pairs(est, ref, return_value=True)
    pair, perm, val = pair.cpu().numpy(), perm.cpu().numpy(), val.cpu().numpy()
    perms = list(itertools.permutations(range(S)))
    B = est.shape[0]
    for b in range(B):
        assert tuple(perm[b]) == perms[int(g[f"upit_idx{S}"][b])]
    want = float(g[f"upit{S}"])
    rel = abs(val.mean() - want) / want
    enh = np.array([pair[:, j, j].sum() / B for j in range(S)])
    rel_e = np.abs(enh - g[f"enh{S}"]) / g[f"enh{S}"]
    print(f"[score] S={S}: loss_uPIT rel {rel:.3e}, loss_Enhance rel {rel_e}")
    assert rel <= 1e-6 and np.all(rel_e <= 1e-6)


@pytest.mark.parametrize("S", [1, 2, 3, 4])
@pytest.mark.parametrize("T", [2, 40, 1001])
def test_spec_pairs_against_numpy(T, S):
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(31 * T + S)
    B, F = 3, 129
    ref = (rng.standard_normal((B, S, T, F)) + 1j * rng.standard_normal((B, S, T, F))).astype(np.complex64)
    sh = list(rng.permutation(S))
    est = (np.float32(0.9) * ref[:, sh] + np.float32(0.1) * (rng.standard_normal((B, S, T, F))
                                                            + 1j * rng.standard_normal((B, S, T, F)))).astype(np.complex64)
    d_e, d_r = torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda()
    pair_t, perm_t, val_t = score.spec_pairs(d_e, d_r, return_value=True)
    again = score.spec_pairs(d_e, d_r, return_value=True)
    assert torch.equal(pair_t, again[0]) and torch.equal(perm_t, again[1]) and torch.equal(val_t, again[2])
    pair, perm, val = pair_t.cpu().numpy(), perm_t.cpu().numpy(), val_t.cpu().numpy()
    for b in range(B):
        want = score_ref.spec_pairs(est[b], ref[b])
        assert np.all(np.abs(pair[b] - want) <= 1e-6 * want), (b, np.abs(pair[b] - want) / want)
        v, p = score_ref.upit(want)
        assert list(perm[b]) == p and abs(val[b] - v) <= 1e-6 * v
        assert list(perm[b]) == [int(x) for x in sh]                       # estimate i belongs to reference sh[i]
    # batch-invariant: item 1 alone, and inside a larger batch at another position; and read in place from a
    # microphone-strided view ([B, S, M, T, F] at one microphone, as the MISO1 estimates lie)
    one = score.spec_pairs(d_e[1:2], d_r[1:2])[0].cpu().numpy()
    assert np.array_equal(one[0], pair[1])
    big_e = torch.from_numpy(np.concatenate([est[::-1], est, est[:1]])).cuda()
    big_r = torch.from_numpy(np.concatenate([ref[::-1], ref, ref[:1]])).cuda()
    big = score.spec_pairs(big_e, big_r)[0].cpu().numpy()
    assert np.array_equal(big[2 * B], pair[0]) and np.array_equal(big[1], pair[1]) and np.array_equal(big[B + 2], pair[2])
    wide = torch.zeros((B, S, 3, T, F), dtype=torch.complex64, device="cuda")
    wide[:, :, 1] = d_e
    assert np.array_equal(score.spec_pairs(wide[:, :, 1], d_r)[0].cpu().numpy(), pair)
    # rectangular: more estimates than references, no pick
    if S >= 2:
        rect, none = score.spec_pairs(d_e, d_r[:, : S - 1])
        assert none is None and np.array_equal(rect.cpu().numpy(), pair[:, :, : S - 1])


@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
@pytest.mark.parametrize("db", [0.0, 20.0, 40.0])
def test_score_waves_known_answer(db, i16):
    """est = swap(clean) * 0.7 + noise: the best permutation is the swap, and SI-SDR / SI-SDRi are score_ref's"""
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(int(db) + 5)
    L = (1 << 20) + 12345                                            # two device pieces
    clean = (0.05 * rng.standard_normal((2, L))).astype(np.float32)
    amp = 0.7 * 0.05 / 10.0 ** (db / 20.0)
    est = (np.float32(0.7) * clean[::-1] + (amp * rng.standard_normal((2, L))).astype(np.float32)).astype(np.float32)
    if i16:
        est = (est * 32767.0).astype(np.int16)
    mix = clean[0] + clean[1]
    sc = score.score_waves(est, clean, mix)
    want = score_ref.score(est, clean, mix)
    print(f"[score] known answer {db:.0f} dB {'int16' if i16 else 'float32'}: si_sdr_best {sc.si_sdr_best} ref {want['si_sdr_best']}"
          f" si_sdri {sc.si_sdri} ref {want['si_sdri']}")
    assert sc.perm_best == [1, 0] == want["perm_best"] and sc.n_samples == L and list(sc.valid) == [True, True]
    assert np.all(np.abs(sc.si_sdr_best - want["si_sdr_best"]) <= DB_TOL)
    assert np.all(np.abs(sc.si_sdr_best - db) <= 0.1)
    assert np.all(np.abs(sc.si_sdr - want["si_sdr"]) <= DB_TOL) and np.all(np.abs(sc.snr - want["snr"]) <= DB_TOL)
    assert np.all(np.abs(sc.si_sdr_mix - want["si_sdr_mix"]) <= DB_TOL)
    assert np.all(np.abs(sc.si_sdri - want["si_sdri"]) <= DB_TOL)
    assert score.score_waves(est, clean).si_sdri is None


def _same_score(a, b):
    da, db_ = a.as_dict(), b.as_dict()
    return json.dumps(da, sort_keys=True) == json.dumps(db_, sort_keys=True)      # repr of every float: bit for bit


def _close_to_ref(sc, want):
    for key in ("si_sdr", "si_sdr_mix", "si_sdri", "snr", "si_sdr_best"):
        got, ref = np.asarray(getattr(sc, key)), np.asarray(want[key])
        print(f"[score] {key}: {got} ref {ref}")
        assert np.all(np.abs(got - ref) <= DB_TOL), key
    assert sc.perm_best == want["perm_best"] and list(sc.valid) == list(want["valid"]) and sc.n_samples == want["n_samples"]


@pytest.mark.parametrize("L", [64000, 150000])
def test_recording_scores(nets, L):
    import misonet_amd as mz
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    obs, s0, s1 = synthetic_utterance(40, L)
    plain = enh.enhance_recording(obs, [s0, s1], max_batch=16)
    seen = []
    for mb in (1, 16):
        pcm, sc = enh.enhance_recording(obs, [s0, s1], max_batch=mb, score=True)
        assert pcm.dtype == np.int16 and np.array_equal(pcm, plain)               # scoring changes no output bit
        assert np.array_equal(enh.enhance_recording(obs, [s0, s1], max_batch=mb), plain)
        _close_to_ref(sc, score_ref.score(pcm, np.stack([s0[:, 0], s1[:, 0]]), obs[:, 0]))
        assert sc.n_samples == L and sc.loss_miso1 is None and sc.loss_enhance is None
        seen.append(sc)
    assert _same_score(seen[0], seen[1])                                          # max_batch moves no bit of the score
    others = [synthetic_utterance(41 + i, n) for i, n in enumerate((70000, 64000, 130001))]
    recs = [(o[0], [o[1], o[2]], f"x{i}") for i, o in enumerate(others)]
    recs.insert(2, (obs, [s0, s1], "me"))
    out = enh.enhance_recordings(recs, max_batch=4, score=True)
    assert list(out) == ["x0", "x1", "me", "x2"]
    assert np.array_equal(out["me"][0], plain) and _same_score(out["me"][1], seen[0])
    off = enh.enhance_recordings(recs, max_batch=4)
    for k in out:
        assert np.array_equal(out[k][0], off[k])


def test_recording_score_needs_clean(nets):
    import misonet_amd as mz
    from misonet_amd.weights import synthetic_utterance
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    obs, s0, s1 = synthetic_utterance(3, 64000)
    with pytest.raises(ValueError):
        enh.enhance_recording(obs, None, score=True)
    with pytest.raises(ValueError):
        enh.enhance_recordings([(obs, [s0, s1], "a"), (obs, None, "b")], score=True)


def _loader():
    from test_gpu_coalesce import _item
    return [_item([200], 2, 300, "a"), _item([201, 202], 1, 100, "b"), _item([203], 3, 1000, "c")]


def _reference_waves(item, b, ref_ch=0):
    """float32 [3, n]: the device iSTFT of the clean spectrograms and of the observation at ref_ch, stitched, gap dropped"""
    from misonet_amd import stft as S
    od, d0, d1, gaps, _ = item
    rows = []
    for d in (d0, d1, od):
        w = [S.istft(d[str(k)][b, ref_ch].cuda()).cpu().numpy() for k in range(len(od))]
        w[-1] = w[-1][: len(w[-1]) - gaps[b]]
        rows.append(np.concatenate(w))
    return np.stack(rows)


def _check_scores_json(save_dir, loader, results, enh=None):
    from misonet_amd import score, stft as S
    with open(os.path.join(save_dir, "scores.json")) as fh:
        doc = json.load(fh)
    names = [n for it in loader for n in it[4]]
    assert sorted(doc) == sorted(names + ["mean"])
    for it in loader:
        for b, name in enumerate(it[4]):
            files = [S.read_wav_pcm24(os.path.join(save_dir, f"{name}_{s}.wav"))[0][:, 0] for s in range(2)]
            est = np.stack([(f >> 8).astype(np.int16) for f in files])
            assert np.array_equal(est, results[name])
            ref = _reference_waves(it, b)
            assert 0 <= est.shape[1] - ref.shape[1] < 64      # the utterance-wise beamformer pads its output to whole hops
            est = est[:, : ref.shape[1]]
            want = score.score_waves(est, ref[:2], ref[2])
            got = doc[name]
            for key in ("si_sdr", "si_sdr_mix", "si_sdri", "snr", "si_sdr_best"):
                print(f"[score] {name} {key}: {got[key]} files {getattr(want, key)}")
                assert np.all(np.abs(np.asarray(got[key]) - getattr(want, key)) <= DB_TOL), (name, key)
            assert got["perm_best"] == want.perm_best and got["n_samples"] == est.shape[1] and got["valid"] == [True, True]
            if enh is not None:
                le, l1 = np.zeros(2), 0.0
                for k in range(len(it[0])):
                    mix = it[0][str(k)][b:b + 1].cuda()
                    clean = torch.stack((it[1][str(k)][b, 0], it[2][str(k)][b, 0]))[None].cuda()
                    out, aux = enh.enhance(mix, clean, want_miso1=True)
                    le += score_ref.loss_enhance(out[0].cpu().numpy(), clean[0].cpu().numpy())
                    l1 += score_ref.upit(score_ref.spec_pairs(aux["miso1"][0, :, 0].cpu().numpy(), clean[0].cpu().numpy()))[0]
                print(f"[score] {name} loss_enhance {got['loss_enhance']} ref {le}; loss_miso1 {got['loss_miso1']} ref {l1}")
                assert np.all(np.abs(np.asarray(got["loss_enhance"]) - le) <= 1e-6 * le)
                assert abs(got["loss_miso1"] - l1) <= 1e-6 * l1
            else:
                assert got["loss_enhance"] is None and got["loss_miso1"] is None
    vals = [v for n in names for v in doc[n]["si_sdr"]]
    assert abs(doc["mean"]["si_sdr"] - np.mean(vals)) <= 1e-9 and doc["mean"]["n_speakers_valid"] == 2 * len(names)


def test_inference_writes_scores(nets, tmp_path):
    import misonet_amd as mz
    m1, m3 = nets
    enh = mz.Enhancer(m1, m3, num_spks=2, ref_ch=0)
    loader = _loader()
    d_off, d_on, d_item = (str(tmp_path / x) for x in ("off", "on", "item"))
    off = enh.inference(loader, d_off)
    assert not os.path.exists(os.path.join(d_off, "scores.json"))
    on = enh.inference(loader, d_on, score=True, max_batch=3)
    assert list(on) == list(off) and all(np.array_equal(on[k], off[k]) for k in off)      # the return value is unchanged
    _check_scores_json(d_on, loader, on, enh)
    per_item = enh.inference(loader, d_item, score=True, coalesce=False)
    assert all(np.array_equal(per_item[k], off[k]) for k in off)
    with open(os.path.join(d_on, "scores.json")) as fa, open(os.path.join(d_item, "scores.json")) as fb:
        assert json.load(fa) == json.load(fb)                                            # the batch moves no bit


def test_testers_pass_score_through(nets, tmp_path):
    from misonet_amd.tester import Tester_Beamforming, Tester_Enhance
    m1, m3 = nets
    loader = _loader()
    args = dict(fs=16000, window="hann", length=256, overlap=192)
    te = Tester_Enhance("SMS_WSJ", "MISO3", loader, loader, m1, m3, 6, 0, 2, 4.0, str(tmp_path), 0, True, **args)
    assert te.score is False
    te.score = True
    d = str(tmp_path / "enh")
    res = te.inference(loader, d)
    _check_scores_json(d, loader, res, te._enh)
    for utt in (False, True):
        tb = Tester_Beamforming("SMS_WSJ", loader, loader, loader, m1, 6, 0, 2, 4.0, str(tmp_path), 0, True, False, utt, **args)
        assert tb.score is False
        d0, d1 = str(tmp_path / f"bf{int(utt)}_off"), str(tmp_path / f"bf{int(utt)}_on")
        want = tb.inference(loader, d0)
        assert not os.path.exists(os.path.join(d0, "scores.json"))
        tb.score = True
        res = tb.inference(loader, d1)
        assert all(np.array_equal(res[k], want[k]) for k in want)
        _check_scores_json(d1, loader, res, None)


def test_hip_graph_capture_of_the_score_calls():
    """one capture of misonet_score_wave + misonet_score_spec: a replay on new inputs gives the bits of the direct calls"""
    _need_gpu()
    from misonet_amd import score
    rng = np.random.default_rng(77)
    B, S, n, T, F = 4, 2, 64000, 40, 129

    def draw():
        est, ref = _signals(rng, B, S, S, n, True)
        z = (rng.standard_normal((2, B, S, T, F)) + 1j * rng.standard_normal((2, B, S, T, F))).astype(np.complex64)
        return torch.from_numpy(est).cuda(), torch.from_numpy(ref).cuda(), torch.from_numpy(z[0]).cuda(), torch.from_numpy(z[1]).cuda()

    e, r, ze, zr = draw()
    nv = torch.tensor([n, n - 7, 100, n], dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        score.wave_stats(e, r, nv)                     # warm the allocator of the capture stream
        score.spec_pairs(ze, zr)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        st = score.wave_stats(e, r, nv)
        pair, perm, val = score.spec_pairs(ze, zr, return_value=True)
    e2, r2, ze2, zr2 = draw()
    for dst, src in ((e, e2), (r, r2), (ze, ze2), (zr, zr2)):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (st, pair, perm, val)]
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, (st, pair, perm, val)))
    want = (score.wave_stats(e2, r2, nv),) + score.spec_pairs(ze2, zr2, return_value=True)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_score_eval_command_line(tmp_path):
    """tools/score_eval.py over two directories of wav files prints what score_waves gives for the same samples"""
    _need_gpu()
    import sys
    from misonet_amd import score, stft as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import score_eval
    rng = np.random.default_rng(9)
    est_dir, ref_dir = tmp_path / "est", tmp_path / "ref"
    est_dir.mkdir()
    ref_dir.mkdir()
    want = {}
    for name, L in (("u1", 70000), ("u2", 64000)):
        cq = (0.05 * 32767 * rng.standard_normal((2, L, 3))).astype(np.int16)            # clean sources, 3 microphones
        eq = (0.6 * cq[:, :, 1] + 40 * rng.standard_normal((2, L))).astype(np.int16)
        mq = (cq[0] + cq[1]).astype(np.int16)
        for s in range(2):
            S.write_wav_pcm24(str(est_dir / f"{name}_{s}.wav"), eq[s], 16000)
            S.write_wav_pcm24(str(ref_dir / f"{name}_{s}.wav"), cq[s], 16000)
        S.write_wav_pcm24(str(ref_dir / f"{name}.wav"), mq, 16000)
        f = lambda q: ((q.astype(np.int32) << 8) / float(1 << 23)).astype(np.float32)   # noqa: E731  (what a wav reader returns)
        want[name] = score.score_waves(eq, f(cq[:, :, 1]), f(mq[:, 1])).as_dict()
    out = tmp_path / "scores.json"
    score_eval.main([str(est_dir), str(ref_dir), "--ref-ch", "1", "--out", str(out)])
    with open(out) as fh:
        doc = json.load(fh)
    assert sorted(doc) == ["mean", "u1", "u2"]
    for name in want:
        assert doc[name] == want[name]
        assert doc[name]["perm_best"] == [0, 1] and min(doc[name]["si_sdri"]) > 5.0
