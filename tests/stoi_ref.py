"""STOI (Taal, Hendriks, Heusdens, Jensen 2011) and ESTOI (Jensen, Taal 2016) restated in NumPy / SciPy, in two independent
forms, plus the test signals of tests/test_stoi.py and tests/test_gpu_stoi.py.  The definition is INTEGRATION.md 4f.

  * :func:`explicit` -- the oracle.  ``scipy.signal.resample_poly`` with the Kaiser window of step 1, the windowed frames
    materialised, the kept ones overlap-added into a signal that is framed again, ``np.fft.rfft``, the segments as one
    array [M, 15, 30] (the way pystoi does it).
  * :func:`direct` -- the form the device computes: the explicit polyphase sum, a new frame formed from its three kept
    neighbours (no overlap-added signal), the band table as bin ranges, one segment at a time.

float64 throughout; an int16 estimate stands for q / 32767.  Both return a dict: stoi, estoi, frames, frames_kept, margin
(min_i |e_i - (max e - 40)| in dB: how far the nearest frame is from flipping), x10 / y10 (the signals at 10 kHz).
"""
import itertools
from math import gcd

import numpy as np
import scipy.signal

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
J = 15
MIN_FREQ = 150.0
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
SHORT = 1e-5                 # the value of a pair with fewer than N_SEG kept frames
RATES = (8000, 10000, 16000)

# band j sums the bins [lo, hi)
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))


def as_f64(est):
    est = np.asarray(est)
    return est.astype(np.float64) / 32767.0 if est.dtype == np.int16 else est.astype(np.float64)


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def band_table():
    """(lo, hi) per band from the third-octave edges, the way the definition derives it"""
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    out = []
    for j in range(J):
        lo = int(np.argmin(np.abs(f - MIN_FREQ * 2.0 ** ((2 * j - 1) / 6.0))))
        hi = int(np.argmin(np.abs(f - MIN_FREQ * 2.0 ** ((2 * j + 1) / 6.0))))
        out.append((lo, hi))
    return tuple(out)


def band_matrix():
    obm = np.zeros((J, NFFT // 2 + 1))
    for j, (lo, hi) in enumerate(band_table()):
        obm[j, lo:hi] = 1.0
    return obm


# ---- step 1: the resampler ---------------------------------------------------------------------------------------------
def resample_filter(fs):
    """(p, q, Lh, h): h the 2 Lh + 1 taps before normalisation"""
    g = gcd(FS, int(fs))
    p, q = FS // g, int(fs) // g
    fc = 1.0 / (2 * max(p, q))
    Lh = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-Lh, Lh + 1)
    h = 2 * p * fc * np.sinc(2 * fc * t) * np.kaiser(2 * Lh + 1, 0.1102 * (60.0 - 8.7))
    return p, q, Lh, h


def resample_scipy(x, fs):
    if int(fs) == FS:
        return np.asarray(x, dtype=np.float64).copy()
    p, q, _, h = resample_filter(fs)
    return scipy.signal.resample_poly(np.asarray(x, dtype=np.float64), p, q, window=h / np.sum(h))


def resample_sum(x, fs, return_abs=False):
    """x10[m] = sum_j x[j] g[m q - j p + Lh], j ascending; ``return_abs``: also sum_j |x[j] g[.]| (the scale of the rounding
    error of any order of summation) and the number of terms"""
    x = np.asarray(x, dtype=np.float64)
    if int(fs) == FS:
        return (x.copy(), np.abs(x), 1) if return_abs else x.copy()
    p, q, Lh, h = resample_filter(fs)
    g = p * h / np.sum(h)
    n = x.shape[0]
    n10 = -(-n * p // q)
    out, mag = np.zeros(n10), np.zeros(n10)
    m = np.arange(n10)
    j_lo = -((Lh - m * q) // p)                                     # ceil((m q - Lh) / p)
    terms = 2 * Lh // p + 1
    for d in range(terms):
        j = j_lo + d
        k = m * q - j * p + Lh
        ok = (j >= 0) & (j < n) & (k >= 0) & (k <= 2 * Lh)
        v = np.where(ok, x[np.clip(j, 0, n - 1)] * g[np.clip(k, 0, 2 * Lh)], 0.0)
        out += v
        mag += np.abs(v)
    return (out, mag, terms) if return_abs else out


# ---- steps 2 .. 7 ------------------------------------------------------------------------------------------------------
def frame_energies(x10):
    w = window()
    nf = (x10.shape[0] - N_FRAME) // HOP + 1 if x10.shape[0] >= N_FRAME else 0
    e = np.array([20.0 * np.log10(np.linalg.norm(w * x10[HOP * i:HOP * i + N_FRAME]) + EPS) for i in range(nf)])
    return e


def kept_frames(x10):
    """(indices of the kept frames, number of frames, margin in dB)"""
    e = frame_energies(x10)
    if e.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), 0, np.inf
    thr = np.max(e) - DYN_RANGE
    return np.nonzero(e > thr)[0], int(e.shape[0]), float(np.min(np.abs(e - thr)))


def _segment_figures(X, Y):
    """X, Y [15, 30] -> (the STOI sum, the ESTOI sum) of one segment"""
    c = np.linalg.norm(X, axis=1, keepdims=True) / (np.linalg.norm(Y, axis=1, keepdims=True) + EPS)
    Yp = np.minimum(c * Y, X * (1.0 + 10.0 ** (-BETA / 20.0)))
    Xc, Yc = X - X.mean(axis=1, keepdims=True), Yp - Yp.mean(axis=1, keepdims=True)
    Xc = Xc / (np.linalg.norm(Xc, axis=1, keepdims=True) + EPS)
    Yc = Yc / (np.linalg.norm(Yc, axis=1, keepdims=True) + EPS)
    d = float(np.sum(Xc * Yc))

    def rc(A):
        A = A - A.mean(axis=1, keepdims=True)
        A = A / (np.linalg.norm(A, axis=1, keepdims=True) + EPS)
        A = A - A.mean(axis=0, keepdims=True)
        return A / (np.linalg.norm(A, axis=0, keepdims=True) + EPS)

    return d, float(np.sum(rc(X) * rc(Y)))


def explicit(x, y, fs):
    """x the clean reference, y the estimate (int16 or float), both [n] at rate fs -> dict"""
    x, y = np.asarray(x, dtype=np.float64), as_f64(y)
    x10, y10 = resample_scipy(x, fs), resample_scipy(y, fs)
    keep, nf, margin = kept_frames(x10)
    K = int(keep.shape[0])
    out = dict(frames=nf, frames_kept=K, margin=margin, x10=x10, y10=y10, stoi=SHORT, estoi=SHORT)
    if K < N_SEG:
        return out
    w = window()
    obm = band_matrix()

    def tob(s10):
        fr = np.array([w * s10[HOP * i:HOP * i + N_FRAME] for i in keep])
        ola = np.zeros(HOP * (K - 1) + N_FRAME)
        for k in range(K):
            ola[HOP * k:HOP * k + N_FRAME] += fr[k]
        spec = np.array([np.fft.rfft(w * ola[HOP * k:HOP * k + N_FRAME], n=NFFT) for k in range(K)]).T      # [257, K]
        return np.sqrt(obm @ np.square(np.abs(spec)))

    tx, ty = tob(x10), tob(y10)
    Xs = np.array([tx[:, m - N_SEG:m] for m in range(N_SEG, K + 1)])                                        # [M, 15, 30]
    Ys = np.array([ty[:, m - N_SEG:m] for m in range(N_SEG, K + 1)])
    M = Xs.shape[0]
    # STOI
    c = np.linalg.norm(Xs, axis=2, keepdims=True) / (np.linalg.norm(Ys, axis=2, keepdims=True) + EPS)
    Yp = np.minimum(Ys * c, Xs * (1.0 + 10.0 ** (-BETA / 20.0)))
    Yp = Yp - np.mean(Yp, axis=2, keepdims=True)
    Xc = Xs - np.mean(Xs, axis=2, keepdims=True)
    Yp = Yp / (np.linalg.norm(Yp, axis=2, keepdims=True) + EPS)
    Xc = Xc / (np.linalg.norm(Xc, axis=2, keepdims=True) + EPS)
    out["stoi"] = float(np.sum(Yp * Xc) / (J * M))

    # ESTOI
    def rc(A):
        A = A - np.mean(A, axis=2, keepdims=True)
        A = A / (np.linalg.norm(A, axis=2, keepdims=True) + EPS)
        A = A - np.mean(A, axis=1, keepdims=True)
        return A / (np.linalg.norm(A, axis=1, keepdims=True) + EPS)

    out["estoi"] = float(np.sum(rc(Xs) * rc(Ys)) / (N_SEG * M))
    return out


def direct(x, y, fs):
    """the same figures the way the device forms them"""
    x, y = np.asarray(x, dtype=np.float64), as_f64(y)
    x10, y10 = resample_sum(x, fs), resample_sum(y, fs)
    keep, nf, margin = kept_frames(x10)
    K = int(keep.shape[0])
    out = dict(frames=nf, frames_kept=K, margin=margin, x10=x10, y10=y10, stoi=SHORT, estoi=SHORT)
    if K < N_SEG:
        return out
    w = window()

    def tob(s10):
        t = np.zeros((J, K))
        for m in range(K):
            cur = w * s10[HOP * keep[m]:HOP * keep[m] + N_FRAME]
            fr = cur.copy()
            if m > 0:
                fr[:HOP] = (w * s10[HOP * keep[m - 1]:HOP * keep[m - 1] + N_FRAME])[HOP:] + cur[:HOP]
            if m + 1 < K:
                fr[HOP:] = cur[HOP:] + (w * s10[HOP * keep[m + 1]:HOP * keep[m + 1] + N_FRAME])[:HOP]
            p2 = np.square(np.abs(np.fft.fft(np.concatenate((w * fr, np.zeros(NFFT - N_FRAME))))[:NFFT // 2 + 1]))
            for j, (lo, hi) in enumerate(BANDS):
                s = 0.0
                for k in range(lo, hi):
                    s += p2[k]
                t[j, m] = np.sqrt(s)
        return t

    tx, ty = tob(x10), tob(y10)
    M = K - N_SEG + 1
    ds = de = 0.0
    for m in range(N_SEG, K + 1):
        a, b = _segment_figures(tx[:, m - N_SEG:m], ty[:, m - N_SEG:m])
        ds += a
        de += b
    out["stoi"], out["estoi"] = ds / (J * M), de / (N_SEG * M)
    return out


def best_perm(M):
    """M [S estimates, S references] -> p, p[j] = the estimate of reference j: the first permutation in itertools order with
    the largest sum_j M[p[j], j]; a non-finite term makes a permutation lose"""
    M = np.asarray(M, dtype=np.float64)
    S = M.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        terms = [M[p[j], j] for j in range(S)]
        v = float(sum(terms)) if all(np.isfinite(t) for t in terms) else -np.inf
        if best is None or v > vbest:
            best, vbest = list(p), v
    return best


def recording(est, clean, mix, fs, form=explicit):
    """est [S, L], clean [S, L], mix [L] or None -> what ``score.stoi_waves`` reports, as a dict of arrays"""
    est, clean = np.asarray(est), np.asarray(clean, dtype=np.float64)
    S = clean.shape[0]
    sm, em = np.zeros((S, S)), np.zeros((S, S))
    frames, kept, margin = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S)
    silent = np.array([not np.sum(clean[j] ** 2) > 0 for j in range(S)])
    for j in range(S):
        for i in range(S):
            r = form(clean[j], est[i], fs)
            sm[i, j] = np.nan if silent[j] else r["stoi"]
            em[i, j] = np.nan if silent[j] else r["estoi"]
            frames[j], kept[j], margin[j] = r["frames"], r["frames_kept"], r["margin"]
    # a reference with K < 30 keeps pystoi's 1e-5 and is not valid; a silent reference is NaN and not valid
    valid = ~silent & (kept >= N_SEG)
    p = best_perm(sm)
    idx = np.arange(S)
    out = dict(stoi=sm[idx, idx], estoi=em[idx, idx], valid=valid, perm_best=p,
               stoi_best=np.array([sm[p[j], j] for j in range(S)]), estoi_best=np.array([em[p[j], j] for j in range(S)]),
               frames=frames, frames_kept=kept, margin=margin, stoi_matrix=sm, estoi_matrix=em,
               stoi_mix=None, estoi_mix=None, stoi_i=None, estoi_i=None)
    if mix is not None:
        rm = [form(clean[j], np.asarray(mix, dtype=np.float64), fs) for j in range(S)]
        out["stoi_mix"] = np.where(silent, np.nan, np.array([r["stoi"] for r in rm]))
        out["estoi_mix"] = np.where(silent, np.nan, np.array([r["estoi"] for r in rm]))
        out["stoi_i"], out["estoi_i"] = out["stoi"] - out["stoi_mix"], out["estoi"] - out["estoi_mix"]
    return out


# ---- the test signals ----------------------------------------------------------------------------------------------------
def speechlike(seed, L, fs, pauses=True):
    """AR(2) noise under a 1.7 Hz envelope with gated pauses (a third of the time 60 dB down, so frames really are removed)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(L + 64)
    s = scipy.signal.lfilter([1.0], [1.0, -1.3, 0.6], e)[64:]
    t = np.arange(L) / float(fs)
    ph = rng.uniform(0, 2 * np.pi)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + ph)
    if pauses:
        gate = (np.sin(2 * np.pi * 0.45 * t + 2.0 * ph) > -0.5).astype(np.float64)
        k = max(1, int(0.01 * fs))
        gate = np.convolve(gate, np.ones(k) / k, mode="same")
        env = env * (1e-3 + (1 - 1e-3) * gate)
    s = s * env
    return (0.25 * s / np.max(np.abs(s))).astype(np.float32)


def case(seed, S, L, fs, snr_db):
    """(est float32 [S, L], clean float32 [S, L], mix float32 [L]): the estimates are the sources plus white noise at snr_db
    and a little of the other speakers"""
    rng = np.random.default_rng(1000 + seed)
    clean = np.stack([speechlike(10 * seed + j, L, fs) for j in range(S)])
    mix = clean.sum(axis=0).astype(np.float32)
    est = np.zeros_like(clean)
    for j in range(S):
        pw = float(np.mean(clean[j].astype(np.float64) ** 2))
        noise = rng.standard_normal(L) * np.sqrt(pw * 10.0 ** (-snr_db / 10.0))
        est[j] = (clean[j] + noise + 0.05 * (mix - clean[j])).astype(np.float32)
    return est, clean, mix


def to_i16(est):
    return np.clip(np.rint(np.asarray(est, dtype=np.float64) * 32767.0), -32768, 32767).astype(np.int16)
