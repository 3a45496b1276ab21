"""CPU tests of the checker of the STFT front end (tests/frontend_ref.py; the device side is tests/test_gpu_stft.py).

(a) the float64 restatement is the reference's contract: ``stft64`` = ``oracle.pipeline_oracle.stft_chunk`` to one complex64
    rounding, ``istft64`` -> int16 = ``pipeline_oracle.istft_int16`` bit for bit outside the near-integer band;
(b) the bars (4 x the float32 statement's own distance from float64, per metric, on the very case) reject what ``stft_pack_k`` and
    ``istft_k`` can get wrong: every planted fault is printed with the metrics that caught it and the factor over the bar;
(c) the int16 band is sound: narrow (at most 5 % of the samples), at a peak of 0.1 ... 0.5 of full scale (at least 3000 LSB), and
    the float32 statement's cast equals the float64 one outside it."""
import functools

import numpy as np
import pytest

import frontend_ref as R
from oracle import pipeline_oracle

EPS32 = 2.0 ** -24


# ----------------------------------------------------------------------------------------------------------------------
# (a)
@pytest.mark.parametrize("L,M", [(64 * 70, 2), (64 * 66 + 17, 3), (300, 1)])
def test_stft64_is_the_scipy_contract(L, M):
    wav = R.wave("white", 1, L, M, seed=1)
    ref = R.stft64(wav)[0]                                              # [M, T, 129] complex128
    T = L // 64 + 1
    assert ref.shape == (M, T, 129)
    # SciPy in float64 (a float32 input makes it transform in float32), cast to complex64 by the oracle; one padded frame more when
    # 64 does not divide L
    sci = pipeline_oracle.stft_chunk(wav[0].astype(np.float64))
    assert sci.shape[1] >= T - 1
    n = min(T, sci.shape[1])
    # one complex64 rounding of each part (half an ulp) + SciPy's own float64 round-off
    tol = 1e-12 * np.abs(ref).max()
    assert np.all(np.abs(sci.real[:, :n] - ref.real[:, :n]) <= EPS32 * np.abs(ref.real[:, :n]) + tol)
    assert np.all(np.abs(sci.imag[:, :n] - ref.imag[:, :n]) <= EPS32 * np.abs(ref.imag[:, :n]) + tol)
    # and the formula in the header of csrc/stft.hip, term by term in float64, on one frame of the second tile
    t = min(T - 1, 65)
    x = np.zeros(128 + 64 * T + 256)
    x[128:128 + L] = wav[0, :, M - 1]
    j = np.arange(256)
    direct = np.array([np.sum(x[64 * t + j] * R.hann64() * np.exp(-2j * np.pi * f * j / 256)) for f in range(129)])
    assert np.abs(direct - ref[M - 1, t]).max() <= 1e-12 * np.abs(direct).max()


@functools.lru_cache(maxsize=None)
def _int16_case(kind, N, T, peak=0.12):
    if kind == "near":
        spec = R.spec_of_wave(R.near_integer_wave(N, 64 * (T - 1), peak=peak))
    else:
        spec = R.scaled_to_peak(R.spectrogram(kind, N, T, amp=1.0) / 3.0 ** np.arange(N)[:, None, None], peak)
    y64 = R.istft64(spec)
    y32 = R.istft32(spec)
    delta, band = R.int16_band(y64, y32)
    return spec, y64, y32, delta, band


@pytest.mark.parametrize("kind", ["white", "near"])
def test_istft64_is_the_scipy_contract(kind):
    spec, y64, _, delta, band = _int16_case(kind, 2, 124)
    for i in range(spec.shape[0]):
        sci = pipeline_oracle.istft_int16(spec[i])
        assert sci.shape == (64 * 123,) and sci.dtype == np.int16
        out, inside, _ = R.int16_verdict(sci, y64[i], band[i])
        assert out == 0 and inside <= 1, (out, inside)


def test_envelope_is_partial_at_both_ends():
    e = R.envelope(6)
    assert abs(e[64:-64] - 1.5).max() < 1e-6 and 1.0 < e[0] < 1.3 and 1.0 < e[-1] < 1.3
    # T = 2: the two frames alone
    assert np.allclose(R.envelope(2), (R.hann64()[128:192] ** 2 + R.hann64()[64:128] ** 2), atol=1e-7)


# ----------------------------------------------------------------------------------------------------------------------
# (b) STFT
def _report(tag, name, ratios, note=""):
    caught = {k: v for k, v in ratios.items() if not v <= 1.0}
    txt = ", ".join(f"{k} x{v:.3g}" for k, v in caught.items()) or "MISSED"
    print(f"[{tag}-fault] {name}: caught by {txt} (factor over the bar){note}")
    return caught


@functools.lru_cache(maxsize=None)
def _stft_case(kind, B, L, M):
    wav = R.wave(kind, B, L, M, seed=2)
    ref = R.stft64(wav)
    f32 = R.stft32(wav)
    return wav, ref, R.stft_metrics(f32, ref), f32


def _stft_faults(wav, f32):
    """name -> faulty output, each through the arithmetic of the float32 statement"""
    B, L, M = wav.shape
    fr = R.frames(wav, dtype=np.float32)
    out = {}
    a = fr.copy()
    a[:, :, 64] = fr[:, :, 65]
    out["frame t = 64 (first of the second tile) from a window one hop late"] = R.stft32(wav, fr=a)
    out["window shifted by one sample"] = R.stft32(wav, fr=R.frames(wav, shift=1, dtype=np.float32))
    out["symmetric hann"] = R.stft32(wav, tables=R.stft_tables(symmetric=True))
    cut = wav.copy()
    cut[:, 64 * (L // 64):] = 0
    out["samples past the last whole hop dropped"] = R.stft32(cut)
    out["front extension by reflection"] = R.stft32(wav, fr=R.frames(wav, reflect=True, dtype=np.float32))
    out["one K step lost (j = 254, 255)"] = R.stft32(wav, ksteps=127)
    a = f32.copy()
    a[..., 37] = f32[..., 38]
    out["bin 37 taken from bin 38"] = a
    a = f32.copy()
    a.imag[..., 0:16] *= -1
    out["imaginary sign in row tile 4 (rows 128..159: f = 128 real, imaginary f = 0..15)"] = a
    a = f32.copy()
    a.imag[..., 112:129] *= -1
    out["imaginary sign in wave 0's third tile (rows 256..272: imaginary f = 112..128)"] = a
    out["microphone m reads m + 1"] = np.roll(f32, -1, axis=1)
    a = f32.copy()
    a[1:] = f32[:-1]
    out["item b reads item b - 1"] = a
    return out


@pytest.mark.parametrize("kind", ["white", "coloured"])
def test_stft_bars_reject_planted_faults(kind):
    wav, ref, m32, f32 = _stft_case(kind, 2, 64 * 65 + 17, 3)            # T = 66: the second tile holds two frames; a tail of 17
    print(f"[stft-f32] {kind}: " + "  ".join(f"{k} {m32[k]:.3e}" for k in R.STFT_KEYS))
    assert m32["zero_ok"] and all(0 < m32[k] < 1e-5 for k in R.STFT_KEYS)
    for name, bad in _stft_faults(wav, f32).items():
        caught = _report("stft", f"{kind}: {name}", R.over_bar(R.stft_metrics(bad, ref), m32, R.STFT_KEYS))
        assert caught, name


def test_stft_healthy_variants_pass():
    """the bars are not so tight that another honest float32 evaluation fails: pairwise products summed in float32 in the reverse
    order of K, and a float64 product rounded once (the best a float32 output can be)"""
    wav, ref, m32, f32 = _stft_case("white", 2, 64 * 65 + 17, 3)
    c, s = R.stft_tables()
    fr = R.frames(wav, dtype=np.float32)
    re = np.zeros(fr.shape[:-1] + (129,), np.float32)
    im = np.zeros_like(re)
    for k in range(254, -2, -2):
        re = (re + fr[..., k + 1, None] * c[k + 1]) + fr[..., k, None] * c[k]
        im = (im + fr[..., k + 1, None] * s[k + 1]) + fr[..., k, None] * s[k]
    rev = re + 1j * im
    once = (fr.astype(np.float64) @ c.astype(np.float64)) + 1j * (fr.astype(np.float64) @ s.astype(np.float64))
    for name, v in (("reverse order", rev), ("float64 product of the float32 tables", once.astype(np.complex64))):
        ratios = R.over_bar(R.stft_metrics(v, ref), m32, R.STFT_KEYS)
        print(f"[stft-healthy] {name}: " + "  ".join(f"{k} {ratios[k] * R.K:.2f}" for k in R.STFT_KEYS) + "  (x the float32 statement)")
        assert all(r <= 1.0 for r in ratios.values()), (name, ratios)


def test_quiet_frame_fault_needs_the_per_frame_metric():
    """A wrong frame t = 64 inside a stretch 160 dB below the rest moves the whole tensor, its bin and its microphone by nothing
    that float32 could see; the frame's own norm convicts it.  This is what the per-frame metric is for."""
    wav, ref, m32, f32 = _stft_case("whisper", 1, 64 * 65 + 17, 2)
    fr = R.frames(wav, dtype=np.float32)
    a = fr.copy()
    a[:, :, 64] = fr[:, :, 65]
    ratios = R.over_bar(R.stft_metrics(R.stft32(wav, fr=a), ref), m32, R.STFT_KEYS)
    caught = _report("stft", "whisper: frame t = 64 from a window one hop late", ratios,
                     "  -- ONLY the per-frame metric sees it" if ratios["whole"] <= 1 else "")
    assert set(caught) == {"frame"}, ratios


def test_silent_frames_are_exact_zeros():
    wav, ref, m32, f32 = _stft_case("silent", 2, 64 * 65 + 17, 3)
    dead = np.sqrt((np.abs(ref) ** 2).sum(-1)) == 0
    assert dead.any() and m32["zero_ok"]
    a = f32.copy()
    b, m, t = np.argwhere(dead)[0]
    a[b, m, t, 5] = 1e-30
    assert not R.stft_metrics(a, ref)["zero_ok"]


# ----------------------------------------------------------------------------------------------------------------------
# (b) iSTFT
@functools.lru_cache(maxsize=None)
def _istft_case(kind, N, T):
    spec = R.spectrogram(kind, N, T, seed=3)
    ref = R.istft64(spec)
    f32 = R.istft32(spec)
    return spec, ref, R.istft_metrics(f32, ref), f32


def _istft_faults(spec):
    nan = np.frombuffer(b"\xff" * 4, np.float32)[0]
    return {
        "c_128 = 2": R.istft32(spec, tables=R.istft_tables(c128=2.0)),
        "c_0 = 2": R.istft32(spec, tables=R.istft_tables(c0=2.0)),
        "envelope 1.5 at both ends": R.istft32(spec, full_env=True),
        "frame j + 2 missing for the last hop of a workgroup (hop 60)": R.istft32(spec, drop=((60, 3),)),
        "frame j - 1 missing for the first hop of the next workgroup (hop 61)": R.istft32(spec, drop=((61, 0),)),
        "imaginary sign flipped": R.istft32(spec, tables=R.istft_tables(flip_im=True)),
        "K rows 258 / 259 hold 0xFF bytes instead of zero": R.istft32(spec, pad_rows=nan),
    }


@pytest.mark.parametrize("kind", ["white", "coloured"])
def test_istft_bars_reject_planted_faults(kind):
    spec, ref, m32, f32 = _istft_case(kind, 2, 64)                      # 63 hops: one workgroup seam, hops 60 | 61
    print(f"[istft-f32] {kind}: " + "  ".join(f"{k} {m32[k]:.3e}" for k in R.ISTFT_KEYS))
    assert all(0 < m32[k] < 2e-6 for k in R.ISTFT_KEYS)
    for name, bad in _istft_faults(spec).items():
        ratios = R.over_bar(R.istft_metrics(bad, ref), m32, R.ISTFT_KEYS)
        only_hop = set(k for k, v in ratios.items() if not v <= 1) == {"hop"}
        caught = _report("istft", f"{kind}: {name}", ratios, "  -- ONLY the per-hop metric sees it" if only_hop else "")
        assert caught, name
    # finite garbage in rows 258 / 259 meets table rows that are zero: harmless, and the statement says so
    assert np.array_equal(R.istft32(spec, pad_rows=np.float32(123.0)), f32)


def test_istft_healthy_variant_passes():
    spec, ref, m32, f32 = _istft_case("white", 2, 64)
    itw, w2 = R.istft_tables()
    b = np.concatenate([spec.real, spec.imag], axis=-1).astype(np.float64)
    z = (b @ itw[:258].astype(np.float64)).astype(np.float32)          # products summed in float64, rounded once
    N, T, _ = z.shape
    zp = np.zeros((N, T + 2, 4, 64), np.float32)
    zp[:, 1:T + 1] = z.reshape(N, T, 4, 64)
    j = np.arange(T - 1)
    tot = sum(zp[:, j + q, 3 - q].astype(np.float64) for q in range(4))
    y = (tot.reshape(N, -1) / R.envelope(T)).astype(np.float32)
    ratios = R.over_bar(R.istft_metrics(y, ref), m32, R.ISTFT_KEYS)
    print("[istft-healthy] float64 sums of the float32 tables: " + "  ".join(f"{k} {ratios[k] * R.K:.2f}" for k in R.ISTFT_KEYS))
    assert all(r <= 1.0 for r in ratios.values()), ratios


# ----------------------------------------------------------------------------------------------------------------------
# (c) the int16 band, and the cast faults
@pytest.mark.parametrize("kind", ["white", "coloured", "silent", "near"])
def test_int16_band_is_sound_and_rejects_wrong_casts(kind):
    spec, y64, y32, delta, band = _int16_case(kind, 2, 124)
    peak = np.abs(y64).max()
    out, inside, share = R.int16_verdict(R.to_int16(y32), y64, band)
    print(f"[int16] {kind}: peak {peak:.3f} of full scale = {peak * 32767:.0f} LSB, delta {delta:.2e} LSB, band holds "
          f"{100 * share:.2f} % of the samples; float32 statement: {out} mismatches outside, max {inside} LSB inside")
    assert 0.1 <= peak <= 0.5 and peak * 32767 >= 3000
    assert share <= 0.05                                                # a condition: an over-wide band could hide a wrong cast
    assert out == 0 and inside <= 1
    for name, q in (("rounding to nearest", R.to_int16(y32, mode="nearest")),
                    ("floor", R.to_int16(y32, mode="floor")),
                    ("full scale 32768", R.to_int16(y32, scale=32768))):
        o, i, _ = R.int16_verdict(q, y64, band)
        print(f"[int16-fault] {kind}: {name}: {o} samples differ outside the band ({100.0 * o / band.size:.1f} %), max {i} LSB inside")
        assert o > 0, name
    if kind == "near":
        # the DC half: values within 0.4 LSB of +3 (even items) and -3 (odd items); floor and truncation part on the negative side
        h = y64.shape[1] // 2
        neg = y64[1, h:] * 32767
        assert np.all(neg < -2.5) and np.all(neg > -3.5) and np.all(y64[0, h:] * 32767 > 2.5)
        assert set(np.unique(R.to_int16(y64[1, h:]))) == {-3, -2} and set(np.unique(R.to_int16(y64[0, h:]))) == {2, 3}
