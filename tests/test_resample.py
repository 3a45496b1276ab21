"""CPU tests of the polyphase resampler: no kernel is launched.  The host side of the C ABI (the ratio, the
lengths, the taps, every rejected argument), the NumPy restatement of tests/resample_ref.py against ``scipy.signal.resample_poly``,
the option validation of the Python entry points, and the bar of the GPU tests against each planted fault.

Figures printed as ``[resample] ...``; LAB.md has them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import resample_ref as R


def _lib():
    from misonet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


NAMES = list(R.RATIOS)


def test_abi_590_symbols():
    L = _lib()
    lib = L.lib()
    for name in ("misonet_resample_ratio", "misonet_resampled_len", "misonet_resample_taps", "misonet_resample_tile",
                 "misonet_resample"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.misonet_version() >= 590
    assert lib.misonet_resample_tile() >= 64
    import misonet_amd as mz
    assert callable(mz.resample) and callable(mz.resampled_len) and callable(mz.load_wav)


@pytest.mark.parametrize("name", NAMES)
def test_ratio_and_taps(name):
    """taps() = firwin(...) p within 1e-14 relative, tap by tap -- at every tap but the zeros of the sinc, the taps at non-zero
    multiples of max(p, q) from the centre (the two end taps among them): there both tables hold 1e-17 of rounding noise of
    sin(k pi), a relative error means nothing, and the bar is absolute, 1e-15 of the largest tap (the noise is 4e-17 of it).
    Also the largest difference over the largest tap, and the rel-L2, within 1e-14."""
    from misonet_amd import resample as RS
    fs_in, fs_out = R.RATIOS[name]
    p, q = R.pq(fs_in, fs_out)
    assert f"{p}/{q}" == name and RS.ratio(fs_in, fs_out) == (p, q)
    want = R.firwin_taps(p, q)
    got = RS.taps(fs_in, fs_out)
    assert got.dtype == np.float64 and got.shape == want.shape == (2 * R.half_len(p, q) + 1,)
    worst, l2 = float(np.max(np.abs(got - want)) / np.max(np.abs(want))), R.rel(got, want)
    print(f"[resample] taps {name}: {got.size} taps, max |diff| / max |g| {worst:.2e}, rel-L2 {l2:.2e}")
    assert worst <= 1e-14 and l2 <= 1e-14
    if name != "1/1":
        k = np.arange(got.size) - R.half_len(p, q)
        zero = (k % max(p, q) == 0) & (k != 0)
        per_tap = float(np.max(np.abs(got - want)[~zero] / np.abs(want[~zero])))
        at_zeros = float(max(np.max(np.abs(got[zero])), np.max(np.abs(want[zero]))) / np.max(np.abs(want)))
        print(f"[resample] taps {name}: worst per-tap relative error {per_tap:.2e} over {int((~zero).sum())} taps; the {int(zero.sum())} "
              f"zeros of the sinc at most {at_zeros:.1e} of the largest tap")
        assert per_tap <= 1e-14 and at_zeros <= 1e-15
    if name == "1/1":
        assert np.array_equal(got, [1.0])


@pytest.mark.parametrize("name", NAMES)
def test_resampled_len_is_scipys(name):
    from scipy.signal import resample_poly
    from misonet_amd import resample as RS
    fs_in, fs_out = R.RATIOS[name]
    p, q = R.pq(fs_in, fs_out)
    lib = _lib().lib()
    got = [lib.misonet_resampled_len(n, fs_in, fs_out) for n in range(1, 2001)]
    assert got == [resample_poly(np.zeros(n), p, q).shape[0] for n in range(1, 2001)]        # SciPy's own, by running it
    assert got == [R.out_len(n, p, q) for n in range(1, 2001)]
    for n in (1, 2, 3, 7, 64, 100, 999, 2000):
        assert got[n - 1] == RS.resampled_len(n, fs_in, fs_out), n
    assert lib.misonet_resampled_len(1 << 28, fs_in, fs_out) == R.out_len(1 << 28, p, q)       # 64-bit arithmetic


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_resample_poly(name):
    """the restatement with SciPy's taps and with the library's, against resample_poly in float64: 1e-13 rel-L2"""
    from misonet_amd import resample as RS
    fs_in, fs_out = R.RATIOS[name]
    p, q = R.pq(fs_in, fs_out)
    for n, M in ((1, 1), (2, 2), (57, 3), (700, 2)):
        x = R.noise(n, M, seed=n).astype(np.float64)
        want = R.oracle(x, p, q)
        a, b = R.restate(x, p, q), R.restate(x, p, q, g=RS.taps(fs_in, fs_out))
        assert a.shape == want.shape == (R.out_len(n, p, q), M)
        ea, eb = R.rel(a, want), R.rel(b, want)
        if n == 700:
            print(f"[resample] restatement {name} n {n}: rel-L2 vs resample_poly {ea:.2e} (SciPy's taps), {eb:.2e} (the library's)")
        assert ea <= 1e-13 and eb <= 1e-13, (n, M, ea, eb)
    one = R.restate(x[:, 0], p, q)
    assert one.ndim == 1 and np.array_equal(one, a[:, 0])


def test_bad_arguments_are_rejected_on_the_host():
    """EINVAL / -1 before any launch and before any pointer is looked at: the pointers given here are not device memory"""
    L = _lib()
    lib = L.lib()
    p, q = C.c_int(), C.c_int()
    assert lib.misonet_resample_ratio(48000, 16000, C.byref(p), C.byref(q)) == 0 and (p.value, q.value) == (1, 3)
    assert lib.misonet_resample_ratio(1024, 1, None, None) == 0 and lib.misonet_resample_ratio(1025, 1, None, None) == L.EINVAL
    assert b"1024" in lib.misonet_last_error()
    for a, b in ((0, 8000), (8000, 0), (-1, 8000), (8000, -5), (44100, 16001), (1, 1025)):
        assert lib.misonet_resample_ratio(a, b, C.byref(p), C.byref(q)) == L.EINVAL, (a, b)
        assert lib.misonet_resampled_len(100, a, b) == -1 and lib.misonet_resample_taps(a, b, None, 0) == L.EINVAL
    assert lib.misonet_resampled_len(0, 16000, 8000) == -1 and lib.misonet_resampled_len(-3, 16000, 8000) == -1
    assert lib.misonet_resampled_len((1 << 28) + 1, 16000, 8000) == -1
    buf = (C.c_double * 41)()
    assert lib.misonet_resample_taps(16000, 8000, None, 0) == 41 and lib.misonet_resample_taps(16000, 8000, buf, 41) == 41
    assert lib.misonet_resample_taps(16000, 8000, buf, 40) == L.EINVAL
    junk = C.c_void_p(16)                                       # never dereferenced
    ok = dict(src=junk, sk=0, ssb=600, ssc=1, sst=6, B=1, M=6, n=100, nv=None, fi=16000, fo=8000, dst=junk, dk=0, dsb=300, dsc=1,
              dst_t=6)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.misonet_resample(a["src"], a["sk"], a["ssb"], a["ssc"], a["sst"], a["B"], a["M"], a["n"], a["nv"], a["fi"],
                                    a["fo"], a["dst"], a["dk"], a["dsb"], a["dsc"], a["dst_t"], None)
    bad = [dict(fi=0), dict(fo=0), dict(fi=1025, fo=1), dict(n=0), dict(n=(1 << 28) + 1), dict(sk=2), dict(sk=-1), dict(dk=2),
           dict(sst=0), dict(sst=-6), dict(ssc=-1), dict(ssb=-1), dict(dst_t=0), dict(dsc=0), dict(B=2, dsb=0), dict(dsb=-1),
           dict(B=0), dict(B=65536), dict(M=0), dict(M=17), dict(src=None), dict(dst=None)]
    for kw in bad:
        assert call(**kw) == L.EINVAL, kw
        assert lib.misonet_last_error() != b""


def test_python_validation_happens_before_any_copy():
    """every rejected option raises without touching the GPU (this test runs where there is none)"""
    from misonet_amd import resample as RS
    x = np.zeros((100, 2), np.float32)
    for a, b in ((0, 8000), (8000, 0), (44100, 16001), (16000.0, 8000), (True, 8000), ("16k", 8000)):
        with pytest.raises(ValueError):
            RS.resample(x, a, b)
        with pytest.raises(ValueError):
            RS.resampled_len(10, a, b)
    with pytest.raises(TypeError):
        RS.resample(x.astype(np.float64), 16000, 8000)
    with pytest.raises(TypeError):
        RS.resample([0.0, 1.0], 16000, 8000)
    with pytest.raises(ValueError):
        RS.resample(np.zeros((2, 3, 4, 5), np.float32), 16000, 8000)
    with pytest.raises(ValueError):
        RS.resample(np.zeros((0, 2), np.float32), 16000, 8000)
    with pytest.raises(ValueError):
        RS.resample(np.zeros((3, 100, 2), np.float32), 16000, 8000, n_valid=[1, 2])
    with pytest.raises(ValueError):
        RS.resample(np.zeros((3, 100, 2), np.float32), 16000, 8000, n_valid=[1, 2, 101])
    with pytest.raises(ValueError):
        RS.resampled_len(0, 16000, 8000)
    assert RS.plan_rates(8000, None, None) == (None, None, 8000) and RS.plan_rates(8000, 8000, "in") == (None, None, 8000)
    assert RS.plan_rates(8000, 16000, "in") == (16000, 16000, 16000) and RS.plan_rates(8000, 16000, None) == (16000, None, 8000)
    assert RS.plan_rates(16000, 48000, 44100) == (48000, 44100, 44100)
    for fi, fo in ((0, None), (None, 0), (None, "out"), (44100, 16001), (None, 8000.5)):
        with pytest.raises(ValueError):
            RS.plan_rates(16000, fi, fo)
    # the recording paths check the rates first: no network, no device and no valid recording is needed to be told
    import misonet_amd as mz
    from misonet_amd.pipeline import Enhancer
    for fn in (Enhancer.enhance_recording, Enhancer.enhance_continuous, mz.BlindSeparator.separate_recording):
        with pytest.raises(ValueError, match="fs_out"):
            fn(None, None, fs=16000, fs_out="native")
    with pytest.raises(ValueError, match="fs_in"):
        Enhancer.enhance_recordings(None, [], fs=16000, fs_in=0)
    with pytest.raises(ValueError, match="fs_in"):
        mz.dereverb_wav(None, fs=16000, fs_in=-1)
    with pytest.raises(ValueError):                             # the SRMR's rates: before the recording is looked at
        mz.dereverb_wav(None, fs=44100, fs_in=48000, srmr=True)


def test_load_wav_reads_pcm16_and_pcm24(tmp_path):
    import wave
    from misonet_amd import resample as RS, stft as S
    q = R.noise(300, 2, seed=3, dtype=np.int16)
    S.write_wav_pcm24(str(tmp_path / "a24.wav"), q, 44100)
    with wave.open(str(tmp_path / "a16.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(22050)
        w.writeframes(q.astype("<i2").tobytes())
    x24, fs24 = RS.load_wav(str(tmp_path / "a24.wav"))
    x16, fs16 = RS.load_wav(str(tmp_path / "a16.wav"), sr=22050)
    assert (fs24, fs16) == (44100, 22050) and x24.dtype == x16.dtype == np.float32 and x24.shape == x16.shape == (300, 2)
    assert np.array_equal(x16, (q / 32768.0).astype(np.float32)) and np.array_equal(x24, x16)      # int16 << 8 over 2^23
    with pytest.raises(ValueError):
        RS.load_wav(str(tmp_path / "a16.wav"), sr=0)


FAULT_CASES = [(name, 6 if name in ("1/2", "160/441") else 2) for name in NAMES if name != "1/1"]


@pytest.mark.parametrize("name,M", FAULT_CASES)
def test_the_bar_rejects_every_planted_fault(name, M):
    """The bar of the GPU tests (within 2 e0 of resample_poly, whole tensor and worst channel) on the float32 rounding of the
    restatement: the clean restatement passes, every planted fault fails -- but for two, which are reported, not asserted:

    ``last_tap`` (the table's entry 2 Lh taken as 0) cannot be caught by any bar: firwin's end taps sit on a zero of the sinc,
    sin(10 pi) / (10 pi) in floating point, |g[2 Lh]| <= 1e-16 max |g| (asserted here), so dropping it changes no float32 bit.
    The tap a walk can really lose is its first or last term: ``j_lo_short`` / ``j_hi_short``, which the bar rejects.

    ``f32_acc`` (float32 products and sums of the 20-110 terms of an output): on these inputs the bar catches it at every ratio
    of the list, but by little -- rel-L2 6.4e-8 (2/1), 6.9e-8 (3/1), 8.2e-8 (147/160), 8.6e-8 (441/160), 9.2e-8 (1/2), 1.2e-7
    (1/3), 1.4e-7 (160/441), 1.7e-7 (80/441) against 2 e0 = 4.8e-8 ... 5.3e-8 -- so the verdict is printed per ratio and not
    asserted: at the short up-sampling filters (21 terms per output at 2/1 and 3/1) another input could leave it inside 2 e0."""
    fs_in, fs_out = R.RATIOS[name]
    p, q = R.pq(fs_in, fs_out)
    n = max(300, 3 * R.half_len(p, q) // p + 50)
    x = R.noise(n, M, seed=11)
    ref64 = R.oracle(x, p, q)
    ok, w, c, ew, ec = R.within_bar(R.restate(x, p, q).astype(np.float32), ref64)
    print(f"[resample] bar {name} M {M} n {n}: clean restatement {w:.3e} / {c:.3e} against 2 e0 = {2 * ew:.3e} / {2 * ec:.3e}")
    assert ok
    g = R.firwin_taps(p, q)
    assert abs(g[-1]) <= 1e-16 * np.max(np.abs(g)) and abs(g[0]) <= 1e-16 * np.max(np.abs(g))
    for fault in R.FAULTS:
        y = R.restate(x, p, q, fault=fault)
        if fault == "swap_pq":
            caught = y.shape != ref64.shape                       # another output length: nothing to compare
            fw = float("nan")
        else:
            passed, fw, fc, _, _ = R.within_bar(y.astype(np.float32), ref64)
            caught = not passed
        print(f"[resample] bar {name} fault {fault}: {'caught' if caught else 'NOT caught'} (rel-L2 {fw:.3e})")
        if fault == "last_tap":
            assert not caught                                     # see above: a fault without an effect
        elif fault != "f32_acc":
            assert caught, fault
