"""STOI / ESTOI on the CPU: the two NumPy forms of tests/stoi_ref.py against each other (the explicit one is the oracle of
tests/test_gpu_stoi.py), the figures of real speech (tests/golden/g16_stoi.npz, written by tools/gen_golden_stoi.py), the host
function ``score.stoi_from_matrices`` against the rules of the edges, and the host side of the C ABI (version 500, the taps,
the size function and its limits).  No device is needed.

Measured: the two forms differ by at most 7.8e-16 in STOI / ESTOI units over all inputs below (FORMS_TOL = ten times that,
rounded up to a power of ten); the library's taps differ from NumPy's by at most 8.9e-16."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import stoi_ref
from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-14     # measured 7.8e-16 (printed below): summation order and the factorisation of the transform
GOLDEN_TOL = 5e-7     # the issue's table carries six decimals


def _golden():
    g = golden("g16_stoi.npz")
    est = g["est_q"].astype(np.float64) / float(1 << 23)
    return g, est, g["clean"], int(g["fs"])


def test_the_two_forms_agree():
    g, est, clean, fs = _golden()
    cases = [("golden0", clean[0], est[0], fs), ("golden1", clean[1], est[1], fs),
             ("golden-crossed", clean[1], est[0], fs), ("golden-mix", clean[0], clean[0] + clean[1], fs)]
    for k, (rate, L, snr) in enumerate(((8000, 24000, 20.0), (10000, 20000, 5.0), (16000, 48000, -5.0), (16000, 30011, 5.0))):
        e, c, m = stoi_ref.case(k, 2, L, rate, snr)
        cases.append((f"ar2 fs={rate} L={L} snr={snr}", c[0], e[0], rate))
        cases.append((f"ar2 fs={rate} L={L} int16", c[1], stoi_ref.to_i16(e[1]), rate))
    worst = 0.0
    for tag, x, y, rate in cases:
        a, b = stoi_ref.explicit(x, y, rate), stoi_ref.direct(x, y, rate)
        assert a["frames"] == b["frames"] and a["frames_kept"] == b["frames_kept"] and a["frames_kept"] >= 30, tag
        d = max(abs(a["stoi"] - b["stoi"]), abs(a["estoi"] - b["estoi"]))
        dx = float(np.abs(a["x10"] - b["x10"]).max())
        print(f"[stoi] {tag}: stoi {a['stoi']:.6f} estoi {a['estoi']:.6f} kept {a['frames_kept']}/{a['frames']} margin "
              f"{a['margin']:.4f} dB; forms differ by {d:.2e}, resampled signals by {dx:.2e}")
        assert d <= FORMS_TOL, (tag, d)
        assert dx <= 1e-13, (tag, dx)                    # the issue: the explicit sum and SciPy agree to 2e-15 at unit scale
        worst = max(worst, d)
    print(f"[stoi] largest gap between the forms {worst:.2e} (asserted {FORMS_TOL:.0e})")


def test_frames_really_are_removed_from_the_synthetic_inputs():
    for fs in stoi_ref.RATES:
        x = stoi_ref.speechlike(3, 4 * fs, fs)
        keep, nf, margin = stoi_ref.kept_frames(stoi_ref.resample_scipy(x, fs))
        assert 30 <= keep.shape[0] < 0.9 * nf, (fs, keep.shape[0], nf)


@pytest.mark.parametrize("fs", stoi_ref.RATES)
def test_a_signal_against_itself_scores_one(fs):
    x = stoi_ref.speechlike(1, 3 * fs, fs)
    for form in (stoi_ref.explicit, stoi_ref.direct):
        r = form(x, x, fs)
        assert abs(r["stoi"] - 1.0) <= 1e-12 and abs(r["estoi"] - 1.0) <= 1e-12, (fs, form.__name__, r["stoi"], r["estoi"])


def test_band_table_and_tap_counts():
    from misonet_amd import score
    assert stoi_ref.band_table() == stoi_ref.BANDS
    assert stoi_ref.BANDS[0] == (7, 9) and stoi_ref.BANDS[-1] == (174, 219) and len(stoi_ref.BANDS) == 15
    assert all(stoi_ref.BANDS[j][1] == stoi_ref.BANDS[j + 1][0] for j in range(14))
    for fs, taps, Lh in ((16000, 581, 290), (8000, 365, 182)):
        p, q, lh, h = stoi_ref.resample_filter(fs)
        assert (lh, h.shape[0]) == (Lh, taps)
        got = score.stoi_taps(fs)
        assert got.shape == (taps,)
        d = float(np.abs(got - p * h / np.sum(h)).max())
        print(f"[stoi] taps of {fs} Hz: library - NumPy {d:.2e}")
        assert d <= 1e-14
    assert np.array_equal(score.stoi_taps(10000), [1.0])
    assert score.stoi_resampled_len(64059, 8000) == 80074 and score.stoi_resampled_len(192000, 16000) == 120000
    assert score.stoi_resampled_len(777, 10000) == 777
    assert score.stoi_resampled_len(100, 44100) < 0 and score.stoi_resampled_len((1 << 24) + 1, 16000) < 0
    # the explicit polyphase sum is scipy.signal.resample_poly
    x = np.random.default_rng(0).standard_normal(5000)
    for fs in (8000, 16000):
        assert np.abs(stoi_ref.resample_sum(x, fs) - stoi_ref.resample_scipy(x, fs)).max() <= 1e-13


def test_golden_figures():
    g, est, clean, fs = _golden()
    assert fs == 8000 and clean.shape == (2, 64059) and clean.dtype == np.float32 and g["est_q"].dtype == np.int32
    want = {(0, 0): (0.977028, 0.942144, 427), (1, 1): (0.971461, 0.922606, 462)}
    for (i, j), (s, e, kept) in want.items():
        r = stoi_ref.explicit(clean[j], est[i], fs)
        assert abs(r["stoi"] - s) <= GOLDEN_TOL and abs(r["estoi"] - e) <= GOLDEN_TOL, (i, j, r["stoi"], r["estoi"])
        assert (r["frames_kept"], r["frames"]) == (kept, 624)
        assert abs(r["stoi"] - g["stoi"][i, j]) <= 1e-12 and abs(r["estoi"] - g["estoi"][i, j]) <= 1e-12     # the recorded oracle
    mix = clean[0].astype(np.float64) + clean[1].astype(np.float64)
    for j, (s, e) in enumerate(((0.733429, 0.577148), (0.707910, 0.541668))):
        r = stoi_ref.explicit(clean[j], mix, fs)
        assert abs(r["stoi"] - s) <= GOLDEN_TOL and abs(r["estoi"] - e) <= GOLDEN_TOL, (j, r["stoi"], r["estoi"])
    assert abs(stoi_ref.explicit(clean[1], est[0], fs)["stoi"] - 0.106) <= 5e-4
    assert float(g["margin"].min()) >= 1e-3 and abs(float(g["margin"][1]) - 0.0148) <= 1e-4


def test_short_and_silent_rules_of_the_restatement():
    fs = 16000
    x = stoi_ref.speechlike(2, 6000, fs, pauses=False)                 # 3750 samples at 10 kHz: 28 frames
    r = stoi_ref.explicit(x, x, fs)
    assert r["frames"] == 28 and r["stoi"] == 1e-5 and r["estoi"] == 1e-5
    assert stoi_ref.explicit(x[:300], x[:300], fs)["frames"] == 0     # below one frame
    est, clean, mix = stoi_ref.case(4, 2, 3 * fs, fs, 5.0)
    clean[1] = 0
    rec = stoi_ref.recording(est, clean, mix, fs)
    assert list(rec["valid"]) == [True, False] and np.isnan(rec["stoi"][1]) and np.isnan(rec["estoi_mix"][1])
    assert np.isfinite(rec["stoi"][0]) and rec["perm_best"] == [0, 1]


def test_from_matrices_rules():
    from misonet_amd import score
    sm = np.array([[0.9, 0.2], [0.1, 0.8]])
    em = np.array([[0.7, 0.1], [0.05, 0.6]])
    st = score.stoi_from_matrices(sm, em, [100, 100], [60, 70], [True, True], [0.5, 0.4], [0.3, 0.2], fs=8000, n_samples=123)
    assert st.perm_best == [0, 1] and np.array_equal(st.stoi, [0.9, 0.8]) and np.array_equal(st.estoi, [0.7, 0.6])
    assert np.array_equal(st.stoi_i, st.stoi - st.stoi_mix) and np.array_equal(st.estoi_i, st.estoi - st.estoi_mix)
    assert list(st.valid) == [True, True] and st.fs == 8000 and st.n_samples == 123
    assert list(st.frames) == [100, 100] and list(st.frames_kept) == [60, 70]
    assert sorted(st.as_dict()) == sorted(["stoi", "estoi", "valid", "perm_best", "stoi_best", "estoi_best", "stoi_mix",
                                           "estoi_mix", "stoi_i", "estoi_i", "frames", "frames_kept", "fs", "n_samples"])
    # swapped estimates: the permutation with the largest summed STOI, and the figures that go with it
    sw = score.stoi_from_matrices(sm[::-1], em[::-1], [100, 100], [60, 70], [True, True])
    assert sw.perm_best == [1, 0] and np.array_equal(sw.stoi_best, [0.9, 0.8]) and np.array_equal(sw.estoi_best, [0.7, 0.6])
    assert sw.stoi_mix is None and sw.stoi_i is None and sw.estoi_i is None
    # ties: the first of the optima in itertools order
    assert score.stoi_from_matrices(np.full((3, 3), 0.5), np.full((3, 3), 0.5), [50] * 3, [40] * 3, [True] * 3).perm_best == [0, 1, 2]
    # fewer than 30 kept frames: 1e-5, not valid; a silent reference: NaN, not valid, and every permutation loses
    sh = score.stoi_from_matrices(sm, em, [29, 100], [29, 70], [True, True], [0.5, 0.4], [0.3, 0.2])
    assert sh.stoi[0] == 1e-5 and sh.estoi[0] == 1e-5 and sh.stoi_mix[0] == 1e-5 and list(sh.valid) == [False, True]
    assert sh.stoi[1] == 0.8
    si = score.stoi_from_matrices(sm[::-1], em[::-1], [100, 100], [100, 70], [False, True], [0.5, 0.4], [0.3, 0.2])
    assert np.isnan(si.stoi[0]) and np.isnan(si.estoi[0]) and np.isnan(si.stoi_mix[0]) and np.isnan(si.stoi_i[0])
    assert list(si.valid) == [False, True] and si.perm_best == [0, 1] and si.stoi[1] == 0.2
    mean = score.stoi_mean_of([st, sh, si])
    assert mean["n_recordings"] == 3 and mean["n_speakers_valid"] == 4
    assert abs(mean["stoi"] - np.mean([0.9, 0.8, 0.8, 0.2])) <= 1e-15
    for p in itertools.permutations(range(3)):                        # the restated rule and the library's agree
        M = np.random.default_rng(sum(p)).uniform(size=(3, 3))
        assert score.best_perm(M) == stoi_ref.best_perm(M)
    with pytest.raises(ValueError):
        score.stoi_from_matrices(np.ones((2, 3)), np.ones((2, 3)), [1, 1], [1, 1], [True, True])
    with pytest.raises(ValueError):
        score.stoi_from_matrices(sm, em, [100], [60, 70], [True, True])
    with pytest.raises(ValueError):
        score.stoi_from_matrices(sm, em, [100, 100], [60, 70], [True, True], stoi_mix=[0.1, 0.1])


def test_value_errors_without_a_device():
    from misonet_amd import score
    x = np.zeros((2, 1000), np.float32)
    for fs in (44100, 48000, 11025, 0, 8000.5):
        with pytest.raises(ValueError, match="8000, 10000 or 16000"):
            score.stoi_waves(x, x, fs=fs)
    with pytest.raises(ValueError):
        score.stoi_waves(np.zeros((5, 1000), np.float32), np.zeros((5, 1000), np.float32), fs=16000)
    with pytest.raises(ValueError):
        score.stoi_unpack(np.zeros(7), 2, 16000, 10)


def test_abi_500_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    new = {"misonet_stoi_scratch_bytes", "misonet_stoi_resample", "misonet_stoi_measure", "misonet_stoi_resampled_len",
           "misonet_stoi_taps"}
    assert new <= declared and declared == set(_lib.SIGNATURES)
    lib = _lib.lib()
    assert lib.misonet_version() >= 500
    for name in new:
        assert hasattr(lib, name)


def test_scratch_bytes_value_and_limits():
    from misonet_amd import score
    for B, NS, R, n10 in itertools.product((1, 16), (2, 3, 5, 9), (1, 2, 4), (1, 255, 256, 4000, 120000, 5 << 22)):
        NE = NS - R
        if not 1 <= NE <= 5:
            assert score.stoi_scratch_bytes(B, NS, R, n10) < 0
            continue
        f = max((n10 - 256) // 128 + 1 if n10 >= 256 else 0, 1)
        want = R * f + 15 * R * (NE + 1) * f + 2 * R * NE * max(f - 29, 1) + R * ((f + 1) // 2)
        assert score.stoi_scratch_bytes(B, NS, R, n10) == 8 * B * want, (B, NS, R, n10)
    good = dict(B=1, NS=5, R=2, n10=1000)
    for key, bad in (("B", (0, -1, 4097)), ("NS", (2, 8)), ("R", (0, 5)), ("n10", (0, -3, (5 << 22) + 1))):
        for v in bad:
            a = dict(good, **{key: v})
            assert score.stoi_scratch_bytes(a["B"], a["NS"], a["R"], a["n10"]) < 0, (key, v)


def test_entry_points_reject_bad_limits_without_a_device():
    """the range checks come before any launch and before the table is built: MISONET_EINVAL with a message"""
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)             # never dereferenced: the checks fail first
    for E, R, n, fs in ((5, 2, 100, 16000), (2, 5, 100, 16000), (2, 0, 100, 8000), (2, 2, (1 << 24) + 1, 16000),
                        (2, 2, 0, 16000), (2, 2, 100, 44100), (2, 2, 100, 0)):
        rc = lib.misonet_stoi_resample(p, 1, n * E, n, 1, p, n * R, n, 1, None, 0, 1, 1, E, R, n, None, fs, p, p, None)
        assert rc == _lib.EINVAL and lib.misonet_last_error(), (E, R, n, fs)
    assert lib.misonet_stoi_resample(p, 1, 200, 100, -1, p, 200, 100, 1, None, 0, 1, 1, 2, 2, 100, None, 8000, p, p, None) \
        == _lib.EINVAL
    assert lib.misonet_stoi_resample(None, 1, 200, 100, 1, p, 200, 100, 1, None, 0, 1, 1, 2, 2, 100, None, 8000, p, p, None) \
        == _lib.EINVAL
    for NS, R, n10 in ((2, 2, 1000), (9, 3, 1000), (3, 0, 1000), (3, 5, 1000), (4, 2, 0), (4, 2, (5 << 22) + 1)):
        assert lib.misonet_stoi_measure(p, None, 1, NS, R, n10, p, p, p, 1 << 40, None) == _lib.EINVAL, (NS, R, n10)
    assert lib.misonet_stoi_measure(p, None, 4097, 4, 2, 1000, p, p, p, 1 << 40, None) == _lib.EINVAL
    assert lib.misonet_stoi_measure(p, None, 1, 4, 2, 120000, p, p, p, 1000, None) == _lib.ENOMEM
    assert lib.misonet_stoi_measure(None, None, 1, 4, 2, 1000, p, p, p, 1 << 40, None) == _lib.EINVAL
    assert lib.misonet_stoi_taps(12345, None) == _lib.EINVAL


def test_against_pystoi_where_it_is_installed():
    """the only permitted skip of this module: pystoi is not a dependency"""
    pystoi = pytest.importorskip("pystoi")
    g, est, clean, fs = _golden()
    for j in range(2):
        r = stoi_ref.explicit(clean[j], est[j], fs)
        x, y = clean[j].astype(np.float64), est[j]
        assert abs(pystoi.stoi(x, y, fs, extended=False) - r["stoi"]) <= 1e-10
        assert abs(pystoi.stoi(x, y, fs, extended=True) - r["estoi"]) <= 1e-10
