"""SRMR on the CPU: the two forms of tests/srmr_ref.py against each other (form (a) is the oracle of tests/test_gpu_srmr.py),
the properties of the definition, the margin condition on every input the GPU test compares, the planted faults against the
ceiling the GPU test asserts, the host side of the C ABI (version 550, the frame, size and chunk functions, the argument checks)
and the host glue of score.py / pipeline.py with ``srmr_measure`` replaced by the oracle.  No device is needed.

Measured: the two forms differ by 1.0e-12 (d64) on 12000 samples at 16 kHz; a change of the envelope by one unit in its last
place alone moves form (a) by 1.4e-12 in the 4 Hz band (the conditioning of that filter in direct form), which is the floor of
any device - oracle deviation.  The planted faults move what the GPU test compares by 1.4e-8 (one float32 rounding of the
envelope, on the single 8 kHz frame; 1.7e-9 on the longer inputs) up to 1 and more; "hop floor for ceil" is not planted: 0.064 fs
is an integer at both rates."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import srmr_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D64_TOL = 1e-10       # the two forms: two float64 / longdouble evaluations of the 4 Hz filter, measured 1e-12


def test_the_two_forms_agree():
    x = sr.signal(16000, 12288, 0.7)[:9000]
    a, b = sr.measure(x, 16000), sr.measure_ld(x, 16000)
    d = sr.deviation(a, b)
    print(f"[srmr] d64 on 9000 samples: {d:.2e}; srmr {a['srmr']:.6f} K* {a['k_star']} BW {a['bw']:.2f}")
    assert a["frames"] == b["frames"] == 5 and d <= D64_TOL, d


def test_design_and_known_properties():
    for fs in sr.RATES:
        d = sr.design(fs)
        assert abs(d["cf"][0] - 125.0) <= 1e-9 and d["cf"][-1] < fs / 2 and np.all(np.diff(d["cf"]) > 0)
        assert d["Nw"] == 256 * fs // 1000 and d["Hw"] == 64 * fs // 1000
        assert abs(d["fk"][0] - 4.0) <= 1e-12 and abs(d["fk"][7] - 128.0) <= 1e-9
        # the response of every channel at its centre is 1
        for j in (0, 11, 22):
            z = np.exp(-2j * np.pi * d["cf"][j] / fs)
            H = d["gain"][j] * np.prod([(d["b"][j, s, 0] + d["b"][j, s, 1] * z) / (1 + d["a"][j, 1] * z + d["a"][j, 2] * z * z)
                                        for s in range(4)])
            assert abs(abs(H) - 1.0) <= 1e-12
        Nw, Hw = d["Nw"], d["Hw"]
        for n, want in ((0, 0), (Nw - 1, 0), (Nw, 1), (Nw + Hw - 1, 1), (Nw + Hw, 2)):
            assert sr.frames_of(n, fs) == want
    with pytest.raises(ValueError):
        sr.design(44100)
    # gain invariance (exact scaling by a power of two; 0.3 within the float32 rounding of the scaled input)
    x = sr.signal(16000, 20011, 0.3)
    base = sr.measure(x, 16000)
    half = sr.measure((0.5 * x).astype(np.float32), 16000)
    assert abs(half["srmr"] - base["srmr"]) <= 1e-12 * base["srmr"] and half["k_star"] == base["k_star"]
    third = sr.measure(0.3 * x.astype(np.float64), 16000)     # as_float64 rounds to float32 once
    assert abs(third["srmr"] - base["srmr"]) <= 1e-5 * base["srmr"]
    # reverberation lowers the figure
    for fs, n in ((16000, 48000), (8000, 30011)):
        dry, wet = sr.oracle_of(fs, n, 0.0, fs == 16000), sr.oracle_of(fs, n, 1.2, fs == 16000)
        assert dry["srmr"] > 1.5 * wet["srmr"], (fs, dry["srmr"], wet["srmr"])
    # too short, and digital silence
    short = sr.measure(x[:4095], 16000)
    assert not short["valid"] and short["frames"] == 0 and np.isnan(short["srmr"]) and short["k_star"] == 0
    silent = sr.measure(np.zeros(5000, np.float32), 16000)
    assert not silent["valid"] and silent["frames"] == 1 and np.isnan(silent["srmr"])


def _all_inputs(chunk):
    for fs in sr.RATES:
        for n, t60 in sr.edge_lengths(fs, chunk):
            yield fs, n, t60, False
    for fs, n, t60s, tmix, i16 in sr.FAMILY:
        for t60 in t60s:
            yield fs, n, t60, i16
        if tmix is not None:
            yield fs, n, tmix, False
    for case in sr.FAULT_INPUTS:
        yield case


def test_margin_on_every_comparison_input():
    """the only discontinuous rule is the 90 % bandwidth: every input the GPU test compares keeps the running sums at j* and
    before it 0.25 points from 90 and BW 1 % from every ll_k"""
    from misonet_amd import score
    chunk = score.srmr_chunk()
    assert chunk == sr.CHUNK                                            # the chunk faults put their seams where the device does
    seen = 0
    for fs, n, t60, i16 in _all_inputs(chunk):
        r = sr.oracle_of(fs, n, t60, i16)
        if n < sr.design(fs)["Nw"]:
            assert not r["valid"]
            continue
        assert sr.margin_ok(r, fs), (fs, n, t60, i16, r["run"], r["bw"])
        seen += 1
    assert seen >= 20
    fs, n, t60 = sr.LONG
    assert sr.margin_ok(sr.oracle_of(fs, n, t60), fs)
    g = np.load(os.path.join(ROOT, "tests", "golden", "g16_stoi.npz"))
    est, mix, fs = sr.golden_signals(g)
    lo, hi = sr.GOLDEN_SLICE
    for x in (est[0], est[1], mix):
        assert sr.margin_ok(sr.measure(x[lo:hi], fs), fs)


@pytest.mark.parametrize("fault", sr.FAULTS)
def test_the_ceiling_rejects_planted_faults(fault):
    """every fault moves what the GPU test compares on at least one of three of its inputs by 100 times the ceiling it asserts
    (a changed K*, frame count or validity counts as infinite: those are compared exactly)"""
    shifts = []
    for fs, n, t60, i16 in sr.FAULT_INPUTS:
        if fault in ("seam_zero", "late_transition") and n <= 2 * sr.CHUNK:
            continue
        if fault == "circular_hilbert" and n & (n - 1) == 0:
            continue
        good, bad = sr.oracle_of(fs, n, t60, i16), sr.measure(sr.signal(fs, n, t60, i16), fs, fault=fault)
        shifts.append(sr.deviation(good, bad))
    print(f"[srmr] fault {fault}: device - oracle would be {max(shifts):.2e} (ceiling {sr.DEV_CEIL:.0e})")
    assert max(shifts) >= 100 * sr.DEV_CEIL, (fault, shifts)


# ---- the host side of the library --------------------------------------------------------------------------------------------
def test_abi_550_header_exports_and_signatures():
    from misonet_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "misonet.h")).read()
    declared = set(re.findall(r"\b(misonet_[a-z0-9_]+)\s*\(", hdr))
    new = {"misonet_srmr_frames", "misonet_srmr_scratch_bytes", "misonet_srmr_chunk", "misonet_srmr_measure"}
    assert new <= declared and new <= set(_lib.SIGNATURES) and "(ABI 550)" in hdr
    lib = _lib.lib()
    assert lib.misonet_version() >= 550
    for name in new:
        assert hasattr(lib, name)


def test_frames_scratch_chunk_and_limits():
    from misonet_amd import score
    C_ = score.srmr_chunk()
    assert C_ >= 1024 and C_ & (C_ - 1) == 0
    for fs in sr.RATES:
        d = sr.design(fs)
        Nw, Hw = d["Nw"], d["Hw"]
        assert C_ % Hw == 0                                             # a hop never straddles a seam
        for n in (0, Nw - 1, Nw, Nw + Hw - 1, Nw + Hw, 1 << 24):
            assert score.srmr_frames(n, fs) == sr.frames_of(n, fs), (n, fs)
        assert score.srmr_frames(-1, fs) < 0 and score.srmr_frames((1 << 24) + 1, fs) < 0
        for B, NS, n in ((1, 1, 100), (1, 1, Nw), (3, 5, 48000), (64, 2, 192000), (4096, 5, 1 << 24)):
            P = 1 << (n - 1).bit_length()
            slot = (n + 1) // 2 * 2 + (2 * P if P > 4096 else 0) + 24 * (-(-n // C_)) + 32 * (-(-n // Hw))
            pairs = B * NS * 23
            groups = max(1, min(pairs, 32768, (1 << 30) // (8 * slot)))
            assert score.srmr_scratch_bytes(B, NS, n, fs) == 8 * (pairs * 8 + groups * slot), (B, NS, n, fs)
        # bounded whatever the batch: 1 GiB of slots (or one slot) and the means
        big = score.srmr_scratch_bytes(4096, 5, 1 << 24, fs)
        assert big <= (1 << 30) + 8 * 4096 * 5 * 184 and score.srmr_scratch_bytes(4096, 5, 192000, fs) <= (1 << 30) + 8 * 4096 * 5 * 184
    assert score.srmr_frames(1000, 10000) < 0 and score.srmr_frames(1000, 44100) < 0
    good = dict(B=1, NS=2, n=1000, fs=8000)
    for key, bad in (("B", (0, -1, 4097)), ("NS", (0, 6)), ("n", (0, -3, (1 << 24) + 1)), ("fs", (0, 10000, 44100))):
        for v in bad:
            a = dict(good, **{key: v})
            assert score.srmr_scratch_bytes(a["B"], a["NS"], a["n"], a["fs"]) < 0, (key, v)


def test_entry_point_rejects_bad_arguments_without_a_device():
    """the checks come before any launch and before the table is built: MISONET_EINVAL / MISONET_ENOMEM with a message"""
    from misonet_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(256)             # never dereferenced: the checks fail first

    def call(sig=p, S=2, n=1000, fs=16000, st=1, out=p, count=p, scratch=p, nbytes=1 << 40, B=1, mix=None, mst=1):
        return lib.misonet_srmr_measure(sig, 1, n * S, n, st, mix, 0, mst, B, S, n, None, fs, out, count, None, scratch, nbytes,
                                        None)

    for kw in (dict(S=5), dict(S=0), dict(n=0), dict(n=(1 << 24) + 1), dict(fs=10000), dict(fs=44100), dict(fs=0), dict(st=-1),
               dict(st=0), dict(sig=None), dict(out=None), dict(count=None), dict(scratch=None), dict(B=0), dict(B=4097),
               dict(mix=p, mst=0)):
        assert call(**kw) == _lib.EINVAL and lib.misonet_last_error(), kw
    assert call(nbytes=1000) == _lib.ENOMEM
    need = lib.misonet_srmr_scratch_bytes(1, 2, 1000, 16000)
    assert call(nbytes=need - 1) == _lib.ENOMEM and need > 0


# ---- the host glue, with the device call replaced by the oracle ---------------------------------------------------------------
class _FakeTensor:
    """what srmr_block's caller does with a device block: index a row, .cpu().numpy()"""
    def __init__(self, a):
        self.a = np.asarray(a)

    def __getitem__(self, i):
        return _FakeTensor(self.a[i])

    def cpu(self):
        return self

    def numpy(self):
        return self.a


def _oracle_block(items, fs):
    rows = []
    for sig, mix in items:
        sig = np.asarray(sig)
        rs = [sr.measure(x, fs) for x in sig] + ([sr.measure(np.asarray(mix), fs)] if mix is not None else [])
        rows.append(np.array([v for r in rs for v in (r["srmr"], r["k_star"], r["bw"])] + [r["frames"] for r in rs], np.float64))
    return _FakeTensor(np.stack(rows))


def test_srmr_waves_and_the_dataclass_on_the_oracle(monkeypatch):
    from misonet_amd import score
    monkeypatch.setattr(score, "srmr_queue", lambda items, fs, dev, pinned=False: _oracle_block(items, fs))
    fs, n = 8000, 14001
    dry, wet = sr.signal(fs, n, 0.0), sr.signal(fs, n, 0.7)
    v = score.srmr_waves(np.stack([dry, wet]), wet, fs=fs, device="cpu")
    od, ow = sr.measure(dry, fs), sr.measure(wet, fs)
    assert isinstance(v, score.Srmr) and v.fs == fs and v.n_samples == n and list(v.valid) == [True, True]
    assert v.srmr[0] == od["srmr"] and v.srmr[1] == ow["srmr"] and v.srmr_mix == ow["srmr"]
    assert list(v.k_star) == [od["k_star"], ow["k_star"]] and v.bw90[0] == od["bw"] and list(v.frames) == [od["frames"]] * 2
    assert v.srmr_i[0] == od["srmr"] - ow["srmr"] > 0 and v.srmr_i[1] == 0.0          # positive is better
    doc = json.loads(json.dumps(v.as_dict()))
    assert doc == v.as_dict() and doc["fs"] == fs and doc["srmr_mix"] == ow["srmr"] and len(doc) == 9
    nomix = score.srmr_waves(np.stack([dry, wet]), None, fs=fs, device="cpu")
    assert nomix.srmr_mix is None and nomix.srmr_i is None and json.loads(json.dumps(nomix.as_dict()))["srmr_i"] is None
    short = score.srmr_waves(dry[None, :2000], dry[:2000], fs=fs, device="cpu")       # shorter than a frame: invalid, no error
    assert list(short.valid) == [False] and np.isnan(short.srmr[0]) and short.k_star[0] == 0 and short.frames[0] == 0
    mean = score.srmr_mean_of([v, nomix, short])
    assert mean["n_recordings"] == 3 and mean["n_signals_valid"] == 4
    assert abs(mean["srmr"] - (od["srmr"] + ow["srmr"]) / 2) <= 1e-12 and abs(mean["srmr_i"] - v.srmr_i.mean()) <= 1e-12
    for bad in (44100, 10000, 0, 8000.5):
        with pytest.raises(ValueError, match="8000 or 16000"):
            score.srmr_waves(dry[None], fs=bad)
        with pytest.raises(ValueError, match="8000 or 16000"):
            score.check_srmr_fs(bad)
    with pytest.raises(ValueError):
        score.srmr_waves(np.zeros((5, 3000), np.float32), fs=8000)                    # S <= 4
    with pytest.raises(ValueError):
        score.srmr_unpack(np.zeros(7), 2, 16000, 10)
    with pytest.raises(ValueError):
        score.srmr_from_rows(np.zeros((2, 4)), np.zeros(2))


def test_the_flag_of_enhance_recording_on_the_oracle(monkeypatch):
    """srmr=True works without score=True and without clean sources, appends last, and leaves the tuple before it alone"""
    from misonet_amd import pipeline, score
    monkeypatch.setattr(score, "srmr_queue", lambda items, fs, dev, pinned=False: _oracle_block(items, fs))
    fs, L = 8000, 6000
    obs = np.stack([sr.signal(fs, L, 0.7), sr.signal(fs, L, 1.2)], axis=1)            # [L, 2 microphones]
    pcm = np.stack([sr.to_i16(sr.signal(fs, L, 0.0)), sr.to_i16(sr.signal(fs, L, 0.3))])
    calls = []

    class Stub(pipeline.Enhancer):
        def __init__(self):
            self.num_ch, self.num_spks, self.ref_ch, self.device, self.dereverb = 2, 2, 1, "cpu", None

    real = pipeline.Enhancer.enhance_recording

    def fake(self, wav_observe, wav_clean=None, *a, **kw):
        if kw.get("srmr"):
            return real(self, wav_observe, wav_clean, *a, **kw)
        calls.append((a, kw))
        score_flag = a[5] if len(a) > 5 else kw.get("score", False)
        return (pcm, "Score") if score_flag else pcm

    monkeypatch.setattr(pipeline.Enhancer, "enhance_recording", fake)
    enh = Stub()
    out = enh.enhance_recording(obs, None, fs=fs, srmr=True)
    assert isinstance(out, tuple) and len(out) == 2 and out[0] is pcm and isinstance(out[1], score.Srmr)
    want = score.srmr_waves(pcm, obs[:, 1], fs=fs, device="cpu")                      # the observation at ref_ch is the mixture
    assert out[1].as_dict() == want.as_dict() and out[1].srmr_mix == sr.measure(obs[:, 1], fs)["srmr"]
    scored = enh.enhance_recording(obs, ["c0", "c1"], fs=fs, score=True, srmr=True)
    assert len(scored) == 3 and scored[0] is pcm and scored[1] == "Score" and scored[2].as_dict() == want.as_dict()
    assert enh.enhance_recording(obs, None, fs=fs) is pcm                              # without the flag: what it always was
    assert all(not kw.get("srmr") for _, kw in calls)
    with pytest.raises(ValueError, match="8000 or 16000"):
        enh.enhance_recording(obs, None, fs=10000, srmr=True)
