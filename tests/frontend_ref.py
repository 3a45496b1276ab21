"""NumPy restatement of the STFT front end and its inverse (csrc/stft.hip: ``stft_pack_k``, ``istft_k``), for
tests/test_frontend.py (CPU) and tests/test_gpu_stft.py (device).  Test infrastructure only.

Two statements of each transform:

  * float64 (``stft64``, ``istft64``): the formula in the header of csrc/stft.hip through NumPy's FFT -- the reference of
    every bound;
  * float32 (``stft32``, ``istft32``): the SAME tables the kernels read (windowed cos / -sin built in float64 with the
    ``(f j) % 256`` argument reduction and rounded to float32; ``c_f / 256`` weights and the float32 ``w^2`` row for the
    inverse), accumulated in float32 sequentially over the K index, two products per step like one 32x32x2 MFMA (128 steps
    forward, 130 inverse), then the four-term float32 overlap-add, the float32 envelope sum and the float32 division of
    ``istft_k``.  Its distance from float64 is "what float32 costs"; a bar is 4 x that figure on the very case, which leaves
    room for the order of additions inside an MFMA and nothing else.  No BLAS: a blocked summation is more accurate than the
    kernel's order and would make the bar too tight for an honest kernel.

The float32 statement takes the faults of tests/test_frontend.py as options, so that the planted fault runs through the same
arithmetic as the healthy statement.  The tables go through ``math.cos`` / ``math.sin`` (the C library's, as the host code of
the kernels) so that the exact-value tests may compare with ``==``."""
import math

import numpy as np

N_FFT, HOP, N_FREQ = 256, 64, 129
IS_K = 260                      # 129 re + 129 im + 2 zero rows
K = 4.0                         # every bar is K x the float32 statement's own figure
MAX_INT16 = 32767


# ----------------------------------------------------------------------------------------------------------------------
# tables
def hann64(symmetric=False):
    n = N_FFT - 1 if symmetric else N_FFT
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * j / n) for j in range(N_FFT)], dtype=np.float64)


_TABLES = {}


def stft_tables(symmetric=False):
    """(cos32, sin32) [256][129] float32: w[j] cos(2 pi f j / 256) and -w[j] sin(2 pi f j / 256) as stft_build_twiddles"""
    key = ("st", symmetric)
    if key not in _TABLES:
        w = hann64(symmetric)
        c = np.empty((N_FFT, N_FREQ), np.float64)
        s = np.empty((N_FFT, N_FREQ), np.float64)
        for j in range(N_FFT):
            for f in range(N_FREQ):
                a = 2.0 * math.pi * float((f * j) % N_FFT) / N_FFT
                c[j, f] = w[j] * math.cos(a)
                s[j, f] = -w[j] * math.sin(a)
        _TABLES[key] = (c.astype(np.float32), s.astype(np.float32))
    return _TABLES[key]


def istft_tables(c0=1.0, c128=1.0, flip_im=False):
    """(itw [260][256], w2 [256]) float32 as istft_build_twiddles: row f < 129 = w[k] c_f / 256 cos, row 129 + f = -w[k] c_f / 256
    sin, rows 258 and 259 zero; w2 = w^2"""
    key = ("is", c0, c128, flip_im)
    if key not in _TABLES:
        w = hann64()
        t = np.zeros((IS_K, N_FFT), np.float64)
        for f in range(N_FREQ):
            cf = c0 if f == 0 else c128 if f == 128 else 2.0
            for k in range(N_FFT):
                a = 2.0 * math.pi * float((f * k) % N_FFT) / 256.0
                t[f, k] = w[k] * cf / 256.0 * math.cos(a)
                t[N_FREQ + f, k] = (w[k] if flip_im else -w[k]) * cf / 256.0 * math.sin(a)
        _TABLES[key] = (t.astype(np.float32), (w * w).astype(np.float32))
    return _TABLES[key]


# ----------------------------------------------------------------------------------------------------------------------
# forward
def n_frames(L):
    return L // HOP + 1


def frames(wav, shift=0, reflect=False, dtype=np.float64):
    """wav [B, L, M] -> [B, M, T, 256]: frame t = samples 64 t - 128 + shift ..., zero outside [0, L) (``reflect``: the front
    extension mirrors the signal instead, a planted fault)"""
    wav = np.asarray(wav)
    B, L, M = wav.shape
    T = n_frames(L)
    x = np.zeros((B, M, 128 + HOP * (T - 1) + N_FFT + 1), dtype)
    x[:, :, 128:128 + L] = wav.transpose(0, 2, 1)
    if reflect:
        n = min(128, L - 1)
        x[:, :, 128 - n:128] = x[:, :, 128 + n:128:-1]
    idx = (HOP * np.arange(T))[:, None] + np.arange(N_FFT)[None, :] + shift
    return x[:, :, idx]


def stft64(wav):
    """wav [B, L, M] -> complex128 [B, M, T, 129], T = L // 64 + 1: zero extension by 128 samples in front and past L, periodic
    hann-256, hop 64, un-normalised"""
    return np.fft.rfft(frames(wav, dtype=np.float64) * hann64(), axis=-1)


def stft32(wav, tables=None, fr=None, ksteps=N_FFT // 2):
    """the float32 statement of stft_pack_k: acc = (acc + a[k] b[k]) + a[k+1] b[k+1] in float32, k = 0, 2, ..., 254"""
    c, s = tables if tables is not None else stft_tables()
    if fr is None:
        fr = frames(np.asarray(wav, np.float32), dtype=np.float32)
    fr = np.ascontiguousarray(fr, np.float32)
    re = np.zeros(fr.shape[:-1] + (N_FREQ,), np.float32)
    im = np.zeros_like(re)
    for k in range(0, 2 * ksteps, 2):
        b0, b1 = fr[..., k, None], fr[..., k + 1, None]
        re = (re + b0 * c[k]) + b1 * c[k + 1]
        im = (im + b0 * s[k]) + b1 * s[k + 1]
    out = np.empty(re.shape, np.complex64)
    out.real, out.imag = re, im
    return out


# ----------------------------------------------------------------------------------------------------------------------
# inverse
def istft64(spec):
    """spec [N, T, 129] -> float64 [N, 64 (T - 1)]: irfft-256, window, overlap-add, division by the true envelope sum w^2
    (partial at both ends, 1.5 inside)"""
    spec = np.asarray(spec).astype(np.complex128)
    N, T, _ = spec.shape
    w = hann64()
    z = np.fft.irfft(spec, n=N_FFT, axis=-1) * w
    n = HOP * (T - 1)
    y = np.zeros((N, n + N_FFT), np.float64)
    env = np.zeros(n + N_FFT, np.float64)
    for t in range(T):
        y[:, HOP * t:HOP * t + N_FFT] += z[:, t]
        env[HOP * t:HOP * t + N_FFT] += w * w
    return y[:, 128:128 + n] / env[128:128 + n]


def istft32_frames(spec, tables=None, pad_rows=None):
    """the windowed inverse DFT of every frame, float32 [N, T, 256]: 130 steps of two products over the rows (re | im | 0 0);
    ``pad_rows`` = what rows 258 and 259 of the operand hold (zeros in the kernel)"""
    itw, _ = tables if tables is not None else istft_tables()
    spec = np.asarray(spec).astype(np.complex64)
    N, T, _ = spec.shape
    b = np.zeros((N, T, IS_K), np.float32)
    b[..., :N_FREQ] = spec.real
    b[..., N_FREQ:2 * N_FREQ] = spec.imag
    if pad_rows is not None:
        b[..., 2 * N_FREQ:] = pad_rows
    z = np.zeros((N, T, N_FFT), np.float32)
    with np.errstate(invalid="ignore"):
        for k in range(0, IS_K, 2):
            z = (z + b[..., k, None] * itw[k]) + b[..., k + 1, None] * itw[k + 1]
    return z


def istft32(spec, tables=None, pad_rows=None, full_env=False, drop=()):
    """the float32 statement of istft_k -> float32 [N, 64 (T - 1)].  Output sample 64 j + m sums the frames j - 1 (k = 192 + m),
    j (128 + m), j + 1 (64 + m), j + 2 (m) in that order, and the envelope the same rows of w^2.
    Faults: ``full_env`` = 1.5 everywhere; ``drop`` = pairs (hop j, q) whose frame j - 1 + q is left out of sum and envelope."""
    _, w2 = tables if tables is not None else istft_tables()
    z = istft32_frames(spec, tables, pad_rows)
    N, T, _ = z.shape
    H = T - 1
    zp = np.zeros((N, T + 2, 4, HOP), np.float32)           # frame t at index t + 1, segment = k // 64
    zp[:, 1:T + 1] = z.reshape(N, T, 4, HOP)
    w2s = w2.reshape(4, HOP)
    total = np.zeros((N, H, HOP), np.float32)
    env = np.zeros((H, HOP), np.float32)
    j = np.arange(H)
    for q in range(4):
        t = j - 1 + q
        ok = (t >= 0) & (t < T)
        for (jd, qd) in drop:
            if qd == q and jd < H:
                ok[jd] = False
        term = zp[:, t + 1, 3 - q] * ok[None, :, None].astype(np.float32)
        total = total + term
        env = env + (np.ones(H, np.float32) if full_env else ok.astype(np.float32))[:, None] * w2s[3 - q][None, :]
    with np.errstate(invalid="ignore"):
        return (total / env[None]).reshape(N, H * HOP).astype(np.float32)


def envelope(T, dtype=np.float64):
    """sum of the float32 w^2 entries over the frames that cover each output sample, evaluated in ``dtype``: [64 (T - 1)]"""
    _, w2 = istft_tables()
    n = HOP * (T - 1)
    env = np.zeros(n + N_FFT, dtype)
    for t in range(T):
        env[HOP * t:HOP * t + N_FFT] += w2.astype(dtype)
    return env[128:128 + n]


def to_int16(y, mode="trunc", scale=MAX_INT16):
    """the cast of istft_k, (short)(int)(y * 32767.0f) in the arithmetic of ``y`` (float32 or float64); ``mode`` / ``scale``: the
    planted faults"""
    y = np.asarray(y)
    v = y * y.dtype.type(scale)
    if mode == "trunc":
        v = np.trunc(v)
    elif mode == "nearest":
        v = np.rint(v)
    elif mode == "floor":
        v = np.floor(v)
    else:
        raise ValueError(mode)
    return v.astype(np.int64).astype(np.int16)


# ----------------------------------------------------------------------------------------------------------------------
# metrics: every figure is ||got - ref64|| over a slice divided by a norm of the reference
def _norm(a, axis):
    return np.sqrt(np.sum(np.abs(a) ** 2, axis=axis))


def _bad(v):
    return float("inf") if not np.isfinite(v) else float(v)


def stft_metrics(got, ref):
    """got, ref complex [B, M, T, 129] -> dict(whole, frame, bin, mic, zero_ok, where).
    frame: each (b, m, t) by its own ||ref|| (frames whose reference is exactly 0 must be exactly 0: ``zero_ok``);
    bin: bin f of item b by sqrt(sum over the item's frames of ||ref frame||^2 / 129), the bin's even share;
    mic: (b, m) by that microphone's ||ref||."""
    got = np.asarray(got).astype(np.complex128)
    ref = np.asarray(ref).astype(np.complex128)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    with np.errstate(invalid="ignore", divide="ignore"):
        rn = _norm(ref, -1)                                  # [B, M, T]
        dn = _norm(d, -1)
        live = rn > 0
        zero_ok = bool(np.all(got[~live] == 0))
        fr = np.where(live, dn / np.where(live, rn, 1.0), 0.0)
        fr = np.where(np.isfinite(fr), fr, np.inf)
        share = np.sqrt(np.sum(rn ** 2, axis=(1, 2)) / N_FREQ)          # [B]
        bn = _norm(d, (1, 2)) / share[:, None]               # [B, 129]
        bn = np.where(np.isfinite(bn), bn, np.inf)
        mic = _norm(d, (2, 3)) / _norm(ref, (2, 3))
        mic = np.where(np.isfinite(mic), mic, np.inf)
        whole = _norm(d, None) / _norm(ref, None)
    return dict(whole=_bad(whole), frame=_bad(fr.max()), bin=_bad(bn.max()), mic=_bad(mic.max()), zero_ok=zero_ok,
                where=dict(frame=tuple(int(i) for i in np.unravel_index(np.argmax(fr), fr.shape)),
                           bin=tuple(int(i) for i in np.unravel_index(np.argmax(bn), bn.shape)),
                           mic=tuple(int(i) for i in np.unravel_index(np.argmax(mic), mic.shape))))


STFT_KEYS = ("whole", "frame", "bin", "mic")


def istft_metrics(got, ref):
    """got, ref [N, 64 H] -> dict(whole, hop, peak, where): whole signal by ||ref||; worst output hop of 64 samples by
    sqrt(||ref item||^2 / H); max |diff| of an item over that item's peak"""
    got = np.asarray(got).astype(np.float64)
    ref = np.asarray(ref).astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    N = ref.shape[0]
    H = ref.shape[1] // HOP
    d = got - ref
    with np.errstate(invalid="ignore", divide="ignore"):
        whole = _norm(d, None) / _norm(ref, None)
        hop = _norm(d.reshape(N, H, HOP), -1) / np.sqrt(np.sum(ref ** 2, axis=1) / H)[:, None]
        hop = np.where(np.isfinite(hop), hop, np.inf)
        peak = np.abs(d).max(axis=1) / np.abs(ref).max(axis=1)
        peak = np.where(np.isfinite(peak), peak, np.inf)
    return dict(whole=_bad(whole), hop=_bad(hop.max()), peak=_bad(peak.max()),
                where=dict(hop=tuple(int(i) for i in np.unravel_index(np.argmax(hop), hop.shape))))


ISTFT_KEYS = ("whole", "hop", "peak")


def over_bar(got_m, f32_m, keys):
    """{metric: got / (K x float32 statement)} -- a value above 1 is over the bar; a statement that is exact (0) admits only 0"""
    out = {}
    for k in keys:
        bar = K * f32_m[k]
        g = got_m[k]
        out[k] = (0.0 if g == 0 else float("inf")) if bar == 0 else (float("inf") if not np.isfinite(g) else g / bar)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the int16 band
def int16_band(ref64, f32):
    """delta = 4 x the float32 statement's max abs error in LSB; band = samples whose float64 value x 32767 sits within delta of
    an integer.  -> (delta, band mask)"""
    v = np.asarray(ref64, np.float64) * MAX_INT16
    delta = K * float(np.abs(np.asarray(f32, np.float64) * MAX_INT16 - v).max())
    return delta, np.abs(v - np.rint(v)) < delta


def int16_verdict(q, ref64, band):
    """q int16 against the float64 cast: (mismatches outside the band, max |diff| inside it, share of the band)"""
    want = to_int16(np.asarray(ref64, np.float64)).astype(np.int32)
    d = np.abs(np.asarray(q).astype(np.int32) - want)
    return int((d[~band] != 0).sum()), int(d[band].max()) if band.any() else 0, float(band.mean())


# ----------------------------------------------------------------------------------------------------------------------
# inputs
KINDS = ("white", "coloured", "silent")


def silent_samples(L):
    """the zero stretches of the 'silent' wave: across the seam of the first 64-frame tile, and the tail"""
    a = [(HOP * 61, min(L, HOP * 67)), (max(0, L - 400), L)]
    return [(lo, hi) for lo, hi in a if lo < hi]


def wave(kind, B, L, M, seed=0, amp=0.02):
    """float32 [B, L, M]; item b is scaled by 3^b so that a wrong item is not a near miss.
    white: noise.  coloured: three low tones (100, 250, 440 Hz at 16 kHz: bins 1.6, 4, 7) with per-microphone phases and noise 60 dB
    below, so the bins differ in energy by orders of magnitude.  silent: white with exact zeros across the tile seam and in the tail.
    whisper: white with the same stretches 160 dB down instead of zero (the CPU test's demonstration of the per-frame metric)."""
    r = np.random.default_rng([seed, B, L, M])
    x = r.standard_normal((B, L, M))
    if kind == "coloured":
        t = np.arange(L)[None, :, None]
        ph = r.uniform(0, 2 * np.pi, (3, B, 1, M))
        tones = sum(a * np.sin(2 * np.pi * f / 16000.0 * t + ph[i]) for i, (f, a) in enumerate([(100.0, 1.0), (250.0, 0.7), (440.0, 0.5)]))
        x = tones + 1e-3 * x
    elif kind in ("silent", "whisper"):
        for lo, hi in silent_samples(L):
            x[:, lo:hi] *= 0.0 if kind == "silent" else 1e-8
    elif kind != "white":
        raise ValueError(kind)
    x *= amp * (3.0 ** np.arange(B))[:, None, None]
    return np.ascontiguousarray(x.astype(np.float32))


def silent_frames(T):
    a = [(59, min(T, 64)), (max(0, T - 3), T)]
    return [(lo, hi) for lo, hi in a if lo < hi]


def spectrogram(kind, N, T, seed=0, amp=1.0):
    """complex64 [N, T, 129] of the same three characters (item n scaled by 3^n): white; coloured = bins 2..6 at 1, the rest 60 dB
    below; silent = white with zero frames across the workgroup seam (59..63: hops 60 and 61 are exact zeros) and in the last three
    frames (the last hop is)"""
    r = np.random.default_rng([seed, N, T, 7])
    z = r.standard_normal((N, T, N_FREQ)) + 1j * r.standard_normal((N, T, N_FREQ))
    if kind == "coloured":
        g = np.full(N_FREQ, 1e-3)
        g[2:7] = 1.0
        z *= g
    elif kind == "silent":
        for lo, hi in silent_frames(T):
            z[:, lo:hi] = 0
    elif kind != "white":
        raise ValueError(kind)
    z *= amp * (3.0 ** np.arange(N))[:, None, None]
    return z.astype(np.complex64)


def scaled_to_peak(spec, peak):
    """the spectrogram scaled (one factor for all items) so that the largest float64 sample of its inverse is ``peak`` of full scale"""
    p = np.abs(istft64(spec)).max()
    return (np.asarray(spec).astype(np.complex128) * (peak / p)).astype(np.complex64)


def near_integer_wave(N, L, seed=0, peak=0.12, dc_lsb=3.0):
    """float64 [N, L] for the int16 cast: first half noise with the given peak (of full scale), second half a DC offset of a few LSB
    (positive for even items, negative for odd ones) with +- 0.4 LSB of uniform noise -- values close to integers on both sides of
    zero, where truncation toward zero, floor and rounding all differ"""
    r = np.random.default_rng([seed, N, L, 11])
    x = r.standard_normal((N, L))
    x *= peak / np.abs(x).max()
    h = L // 2
    sign = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)[:, None]
    x[:, h:] = (sign * dc_lsb + r.uniform(-0.4, 0.4, (N, L - h))) / MAX_INT16
    return x


def spec_of_wave(x):
    """[N, L] float64, L a multiple of 64 -> complex64 [N, L / 64 + 1, 129] whose inverse is x"""
    return stft64(np.asarray(x)[:, :, None])[:, 0].astype(np.complex64)
