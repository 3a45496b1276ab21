"""Cepstral distance, LLR and fwSegSNR on the CPU: the two NumPy forms of tests/reverb_ref.py against each other (the explicit
one is the oracle of tests/test_gpu_reverb.py), known answers, the condition that no frame of the GPU test's inputs is dropped,
the planted faults against the bound the GPU test asserts, and the host side of the C ABI (version 540, the frame and size
functions, the argument checks).  No device is needed.

Measured: the two forms differ by at most 4.5e-11 (the LLR of one frame of the real speech; 1.4e-12 on the synthetic inputs)
over every figure and every value of every frame of the GPU test's inputs; the issue's bound is 1e-10."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import reverb_ref as rr
import stoi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS_TOL = 1e-10     # set by the issue


@pytest.mark.parametrize("tag", ["golden"] + [f"case{k}" for k in range(len(rr.CASES))])
def test_the_two_forms_agree_and_no_frame_is_dropped(tag):
    est, clean, mix, fs = rr.inputs()[tag]
    a, b = rr.oracle(tag), rr.recording(est, clean, mix, fs, form="direct")
    assert np.array_equal(a["counts"], b["counts"]) and a["perm_best"] == b["perm_best"]
    d = rr.deviation(a, b)
    print(f"[reverb] {tag}: cd {a['cd']} llr {a['llr']} fwsegsnr {a['fwsegsnr']} frames {a['frames']}; forms differ by {d:.2e}")
    assert d <= FORMS_TOL, (tag, d)
    # the cap that keeps the comparison on the device from hiding frames: every frame is used and counts for LLR, in every
    # pair (the clips are continuous, so a value on one needs no margin)
    nfr = rr.frames_of(clean.shape[1], fs)
    assert nfr > 0 and np.all(a["counts"] == nfr), (tag, a["counts"])
    assert np.all(a["valid"]) and not np.isnan(a["frame_values"]).any()


@pytest.mark.parametrize("fs", rr.RATES)
def test_known_answers(fs):
    N, H, _ = rr.geometry(fs)
    x = stoi_ref.speechlike(3, 2 * fs, fs)
    y = stoi_ref.case(5, 1, 2 * fs, fs, 10.0)[0][0]
    nfr = rr.frames_of(2 * fs, fs)
    # a signal against itself
    r = rr.explicit(x, x, fs)
    assert r["K"] == r["K_llr"] == r["frames"] == nfr and r["valid"]
    assert r["cd"] == 0.0 and r["cd_median"] == 0.0 and r["llr"] == 0.0 and r["llr_median"] == 0.0
    assert r["fwsegsnr"] == 35.0 and r["fwsegsnr_median"] == 35.0
    # the gain of either signal moves nothing beyond the float32 rounding of the scaled input (2^-24 relative per sample)
    base = rr.explicit(x, y, fs)
    for xs, ys in ((0.3, 1.0), (1.0, 0.3)):
        exact = rr.explicit(xs * x.astype(np.float64), ys * y.astype(np.float64), fs)
        rounded = rr.explicit((xs * x).astype(np.float32), (ys * y).astype(np.float32), fs)
        for key in rr.FIGURES:
            assert abs(exact[key] - base[key]) <= 1e-9, (key, xs, ys)
            assert abs(rounded[key] - base[key]) <= 2e-3, (key, xs, ys)
    # y = 0: fwSegSNR exactly 0, no frame counts for LLR
    z = rr.explicit(x, np.zeros_like(x), fs)
    assert z["fwsegsnr"] == 0.0 and z["fwsegsnr_median"] == 0.0 and z["K_llr"] == 0 and z["K"] == nfr
    assert np.isnan(z["llr"]) and np.isnan(z["llr_median"]) and np.isfinite(z["cd"])
    # a run of exact zeros in the reference drops exactly the frames that lie inside it
    xz = x.copy()
    lo, hi = 10 * H, 10 * H + 5 * H + N
    xz[lo:hi] = 0.0
    d = rr.explicit(xz, y, fs)
    gone = np.nonzero(np.isnan(d["cd_t"]))[0]
    assert list(gone) == list(range(10, 16)) and d["K"] == nfr - 6 and d["frames"] == nfr
    assert np.array_equal(np.isnan(d["fw_t"]), np.isnan(d["cd_t"])) and np.all(np.isnan(d["llr_t"][gone]))
    # a silent reference, and fewer samples than a frame
    s = rr.explicit(np.zeros_like(x), y, fs)
    assert not s["valid"] and s["K"] == 0 and all(np.isnan(s[k]) for k in rr.FIGURES)
    short = rr.explicit(x[:N - 1], y[:N - 1], fs)
    assert short["frames"] == 0 and not short["valid"] and all(np.isnan(short[k]) for k in rr.FIGURES)
    for n, want in ((N - 1, 0), (N, 1), (N + H - 1, 1), (N + H, 2)):
        assert rr.frames_of(n, fs) == want


def test_medians():
    assert rr.median([3.0]) == 3.0 and rr.median([4.0, 1.0]) == 2.5 and rr.median([9.0, 1.0, 4.0]) == 4.0
    assert rr.median([8.0, 1.0, 2.0, 4.0]) == 3.0 and np.isnan(rr.median([]))
    fs = 8000
    N, H, _ = rr.geometry(fs)
    x, y = stoi_ref.speechlike(1, N + 3 * H, fs, pauses=False), stoi_ref.speechlike(2, N + 3 * H, fs, pauses=False)
    for K in (1, 2, 3, 4):
        n = N + (K - 1) * H
        r = rr.explicit(x[:n], y[:n], fs)
        v = np.sort(r["fw_t"])
        assert r["K"] == K and r["fwsegsnr_median"] == (v[(K - 1) // 2] if K % 2 else (v[K // 2 - 1] + v[K // 2]) / 2.0)


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_the_bound_rejects_planted_faults(fault):
    """every fault moves what the GPU test compares (the figures of every pair and the values of every frame, or a count, which
    it compares exactly) by more than the ceiling it asserts, on each of two of its inputs; case 1 has an even number of frames,
    so the even median is exercised there"""
    assert rr.DEV_CEIL <= 1e-9
    for tag in ("case1", "case4"):
        est, clean, mix, fs = rr.inputs()[tag]
        good, bad = rr.oracle(tag), rr.recording(est, clean, mix, fs, **{fault: True})
        if fault == "upper_median" and good["frames"][0] % 2:
            continue
        d = rr.deviation(good, bad) if np.array_equal(good["counts"], bad["counts"]) else np.inf
        print(f"[reverb] fault {fault} on {tag}: device - oracle would be {d:.2e} (ceiling {rr.DEV_CEIL:.0e})")
        assert d > 10 * rr.DEV_CEIL, (fault, tag, d)


def test_unknown_rate():
    with pytest.raises(ValueError):
        rr.geometry(10000)


# ---- the host side of the library --------------------------------------------------------------------------------------------
def test_abi_540_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    new = {"misonet_reverb_frames", "misonet_reverb_scratch_bytes", "misonet_reverb_measure"}
    assert new <= declared and new <= set(_lib.SIGNATURES) and "(ABI 540)" in hdr
    lib = _lib.lib()
    assert lib.misonet_version() >= 540
    for name in new:
        assert hasattr(lib, name)


def test_frames_scratch_and_limits():
    from misonet_amd import score
    for fs in rr.RATES:
        N, H, _ = rr.geometry(fs)
        for n in (1, N - 1, N, N + H - 1, N + H, 23456, 82120, 1 << 24):
            assert score.reverb_frames(n, fs) == rr.frames_of(n, fs), (n, fs)
        assert score.reverb_frames(0, fs) < 0 and score.reverb_frames((1 << 24) + 1, fs) < 0
        for B, NS, R, n in ((1, 2, 1, 100), (3, 5, 2, 48000), (16, 9, 4, 82120), (4096, 3, 1, N)):
            f = max(rr.frames_of(n, fs), 1)
            assert score.reverb_scratch_bytes(B, NS, R, n, fs) == 8 * B * (NS + 75 * NS * f + 3 * (NS - R) * R * f)
    assert score.reverb_frames(1000, 10000) < 0 and score.reverb_frames(1000, 44100) < 0
    good = dict(B=1, NS=5, R=2, n=1000, fs=8000)
    for key, bad in (("B", (0, -1, 4097)), ("NS", (2, 8)), ("R", (0, 5)), ("n", (0, -3, (1 << 24) + 1)), ("fs", (0, 10000, 44100))):
        for v in bad:
            a = dict(good, **{key: v})
            assert score.reverb_scratch_bytes(a["B"], a["NS"], a["R"], a["n"], a["fs"]) < 0, (key, v)


def test_entry_point_rejects_bad_arguments_without_a_device():
    """the checks come before any launch and before the table is built: MISONET_EINVAL / MISONET_ENOMEM with a message"""
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)             # never dereferenced: the checks fail first

    def call(est=p, E=2, R=2, n=1000, fs=16000, st=1, out=p, count=p, scratch=p, nbytes=1 << 40, B=1, mix=None, mst=1):
        return lib.misonet_reverb_measure(est, 1, n * E, n, st, p, n * R, n, 1, mix, 0, mst, B, E, R, n, None, fs, out, count,
                                          None, scratch, nbytes, None)

    for kw in (dict(E=5), dict(E=0), dict(R=5), dict(R=0), dict(n=0), dict(n=(1 << 24) + 1), dict(fs=10000), dict(fs=44100),
               dict(fs=0), dict(st=-1), dict(st=0), dict(est=None), dict(out=None), dict(count=None), dict(scratch=None),
               dict(B=0), dict(B=4097), dict(mix=p, mst=0)):
        assert call(**kw) == _lib.EINVAL and lib.misonet_last_error(), kw
    assert call(nbytes=1000) == _lib.ENOMEM
    need = lib.misonet_reverb_scratch_bytes(1, 4, 2, 1000, 16000)
    assert call(nbytes=need - 1) == _lib.ENOMEM and need > 0


def test_value_errors_and_the_dataclass_without_a_device():
    from misonet_amd import score
    x = np.zeros((2, 1000), np.float32)
    for fs in (44100, 10000, 0, 8000.5):
        with pytest.raises(ValueError, match="8000 or 16000"):
            score.reverb_waves(x, x, fs=fs)
        with pytest.raises(ValueError, match="8000 or 16000"):
            score.check_reverb_fs(fs)
    with pytest.raises(ValueError):
        score.reverb_waves(np.zeros((5, 1000), np.float32), np.zeros((5, 1000), np.float32), fs=16000)
    with pytest.raises(ValueError):
        score.reverb_unpack(np.zeros(7), 2, 16000, 10)
    # the dataclass from the oracle's matrices: the same figures, and a JSON round trip
    est, clean, mix, fs = rr.inputs()["case0"]
    want = rr.oracle("case0")
    S = clean.shape[0]
    row = np.concatenate([want["matrix"].ravel(), want["counts"].astype(np.float64).ravel()])
    rv = score.reverb_unpack(row, S, fs, clean.shape[1])
    for key in rr.FIGURES:
        for suffix in ("", "_best", "_mix", "_i"):
            assert np.array_equal(getattr(rv, key + suffix), want[key + suffix]), key + suffix
    assert rv.perm_best == want["perm_best"] and list(rv.frames_used) == list(want["frames_used"]) and all(rv.valid)
    doc = json.loads(json.dumps(rv.as_dict()))
    assert doc == rv.as_dict() and doc["fs"] == fs and doc["n_samples"] == clean.shape[1] and len(doc) == 24 + 7
    swapped = score.reverb_unpack(np.concatenate([want["matrix"][[1, 0, 2]].ravel(), want["counts"].astype(np.float64).ravel()]),
                                  S, fs, clean.shape[1])
    assert swapped.perm_best == [1, 0] and np.array_equal(swapped.cd_best, rv.cd) and np.array_equal(swapped.cd_i, rv.cd_i)
    nomix = score.reverb_unpack(row.reshape(-1)[np.r_[0:6 * S * S, 6 * S * (S + 1):6 * S * (S + 1) + 3 * S * S]], S, fs, 10)
    assert nomix.cd_mix is None and nomix.fwsegsnr_i is None and json.loads(json.dumps(nomix.as_dict()))["cd_mix"] is None
    mean = score.reverb_mean_of([rv, swapped])
    assert mean["n_recordings"] == 2 and mean["n_speakers_valid"] == 2 * S and abs(mean["cd_best"] - np.mean(rv.cd)) <= 1e-12
    with pytest.raises(ValueError):
        score.reverb_from_matrices(np.zeros((2, 3, 6)), np.zeros((2, 3, 3)))
