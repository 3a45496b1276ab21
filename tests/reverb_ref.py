"""Cepstral distance, log-likelihood ratio and frequency-weighted segmental SNR restated in float64 NumPy,
in two independent forms, plus the inputs shared by tests/test_reverb.py and tests/test_gpu_reverb.py.

  * :func:`explicit` -- the oracle.  ``np.fft.rfft``, the cepstrum through a cosine matrix, the mel triangles from the min / max
    formula, the lags as sliced dot products, Levinson-Durbin, Q(a, r) as a double sum over the lags.
  * :func:`direct` -- the explicit DFT sum (accumulated in ``np.longdouble``), the cepstrum as ``np.fft.ifft(l).real[:25]``, the triangles by interpolation between
    the edges, the lags from ``np.correlate``, the LPC by ``np.linalg.solve`` on the Toeplitz normal equations, Q through the
    explicit matrix.

The features of a signal (:func:`features`) are computed once and shared by every pair it takes part in, as on the device.  An
int16 estimate stands for q / 32767.  Every keyword of ``FAULTS`` plants one fault into the explicit form: tests/test_reverb.py
shows that the bound the GPU test asserts rejects each of them.
"""
import itertools

import numpy as np

import stoi_ref

RATES = (8000, 16000)
NQ = 25                  # cepstral coefficients 0 .. 24
NB = 23                  # mel bands
ORDER = 12               # LPC order
FLOOR = 1e-15
CD_CAP = 10.0
LLR_CAP = 2.0
SNR_LO, SNR_HI = -10.0, 35.0
FIGURES = ("cd", "cd_median", "llr", "llr_median", "fwsegsnr", "fwsegsnr_median")

# device - oracle over every input of tests/test_gpu_reverb.py, in dB (CD, fwSegSNR) and nats (LLR): ten times the largest
# deviation measured on an MI355X (4.7e-11, on the real speech; 6.4e-14 on the synthetic inputs), rounded up to a power of ten;
# the condition the issue sets on it is <= 1e-9
DEV_CEIL = 1e-9

FAULTS = ("hanning_zero", "no_mean_norm", "lpc10", "no_factor2", "mel_shift", "drop_last", "upper_median", "no_gain",
          "circular_r", "f32_frame")

# (fs, L, S, SNR of the added noise in dB, int16 estimates): the synthetic inputs of the GPU test
CASES = [(16000, 48000, 2, 5.0, True), (16000, 30011, 1, 20.0, False), (16000, 64000, 3, 35.0, True),
         (8000, 40000, 3, 5.0, False), (8000, 23456, 2, 20.0, True), (8000, 33333, 1, 35.0, False)]


def synthetic(k):
    fs, L, S, snr, i16 = CASES[k]
    est, clean, mix = stoi_ref.case(40 + k, S, L, fs, snr)
    return (stoi_ref.to_i16(est) if i16 else est), clean, mix, fs


GOLDEN_START = 3600      # the first reference of the golden recording is digital silence up to sample 3571


def golden_case(g):
    """the real speech of tests/golden/g16_stoi.npz (8 kHz) from sample GOLDEN_START on, so that no frame is dropped: (est
    float32 [2, L] from the 24-bit integers, exact in float32; clean float32 [2, L]; mix float32 [L]; fs)"""
    est = (g["est_q"].astype(np.float64) / float(1 << 23)).astype(np.float32)[:, GOLDEN_START:]
    clean = g["clean"][:, GOLDEN_START:]
    return np.ascontiguousarray(est), np.ascontiguousarray(clean), (clean[0] + clean[1]).astype(np.float32), int(g["fs"])


def geometry(fs):
    """(N, H, NFFT)"""
    if int(fs) not in RATES:
        raise ValueError(f"fs must be 8000 or 16000 (got {fs})")
    return int(fs) // 40, int(fs) // 100, 256 if int(fs) == 8000 else 512


def frames_of(n, fs):
    N, H, _ = geometry(fs)
    return (n - N) // H + 1 if n >= N else 0


def window(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(N) + 1) / (N + 1))


def mel_edges(fs):
    top = 2595.0 * np.log10(1.0 + 0.5 * fs / 700.0)
    return 700.0 * (10.0 ** (top * np.arange(NB + 2) / (NB + 1) / 2595.0) - 1.0)


def mel_matrix(fs, NFFT):
    """H [23, NFFT / 2 + 1] from the min / max formula"""
    e = mel_edges(fs)
    f = np.arange(NFFT // 2 + 1) * float(fs) / NFFT
    return np.array([np.maximum(0.0, np.minimum((f - e[b]) / (e[b + 1] - e[b]), (e[b + 2] - f) / (e[b + 2] - e[b + 1])))
                     for b in range(NB)])


def mel_matrix_interp(fs, NFFT):
    e = mel_edges(fs)
    f = np.arange(NFFT // 2 + 1) * float(fs) / NFFT
    return np.array([np.interp(f, e[b:b + 3], [0.0, 1.0, 0.0], left=0.0, right=0.0) for b in range(NB)])


def levinson(r, order):
    """r [T, >= order + 1] -> (a [T, order + 1] with a[:, 0] = 1, failed [T]): failed where some E_0 .. E_order is <= 0 or not
    finite (the coefficients of a failed frame are not used)"""
    T = r.shape[0]
    a = np.zeros((T, order + 1))
    a[:, 0] = 1.0
    err = r[:, 0].copy()
    fail = ~(err > 0) | ~np.isfinite(err)
    with np.errstate(all="ignore"):
        for k in range(1, order + 1):
            acc = np.zeros(T)
            for j in range(k):
                acc = acc + a[:, j] * r[:, k - j]
            lam = np.where(fail, 0.0, -acc / np.where(fail, 1.0, err))
            a[:, :k + 1] = a[:, :k + 1] + lam[:, None] * a[:, k::-1]
            err = err * (1.0 - lam * lam)
            fail = fail | ~(err > 0) | ~np.isfinite(err)
    return a, fail


def lpc_solve(r, order):
    """the same coefficients from the Toeplitz normal equations; failed where r[0] <= 0, the system is singular or the
    prediction error r[0] + sum_k a[k] r[k] is <= 0 or not finite"""
    T = r.shape[0]
    a = np.zeros((T, order + 1))
    a[:, 0] = 1.0
    fail = np.zeros(T, dtype=bool)
    i = np.arange(order)
    for t in range(T):
        if not r[t, 0] > 0:
            fail[t] = True
            continue
        try:
            a[t, 1:] = np.linalg.solve(r[t][np.abs(i[:, None] - i[None, :])], -r[t, 1:order + 1])
        except np.linalg.LinAlgError:
            fail[t] = True
            continue
        e = float(np.dot(a[t], r[t, :order + 1]))
        fail[t] = not (e > 0 and np.isfinite(e))
    return a, fail


def features(x, fs, form="explicit", **faults):
    """x [n] (int16 or float) -> dict: nfr, P, X [nfr, NFFT / 2 + 1], c [nfr, 25], B [nfr, 23], r [nfr, 13], a [nfr, 13], fail"""
    x = stoi_ref.as_f64(x)
    N, H, NFFT = geometry(fs)
    n = x.shape[0]
    nfr = frames_of(n, fs)
    if faults.get("drop_last") and nfr > 0:
        nfr -= 1
    order = 10 if faults.get("lpc10") else ORDER
    w = np.hanning(N) if faults.get("hanning_zero") else window(N)
    u = w[None, :] * x[(np.arange(nfr) * H)[:, None] + np.arange(N)[None, :]] if nfr else np.zeros((0, N))
    if faults.get("f32_frame"):
        u = u.astype(np.float32).astype(np.float64)
    nbin = NFFT // 2 + 1
    if form == "explicit":
        X = np.abs(np.fft.rfft(u, n=NFFT, axis=1))
        ell = np.log(np.maximum(X, FLOOR))
        full = np.concatenate([ell, ell[:, NFFT // 2 - 1:0:-1]], axis=1)                       # extended evenly to m < NFFT
        cosm = np.cos(2.0 * np.pi * np.outer(np.arange(NFFT), np.arange(NQ)) / NFFT)
        c = full @ cosm / NFFT
        Hm = mel_matrix(fs, NFFT)
        if faults.get("mel_shift"):
            Hm = np.concatenate([np.zeros((NB, 1)), Hm[:, :-1]], axis=1)
        B = X @ Hm.T
        if faults.get("circular_r"):
            r = np.stack([np.sum(u * np.roll(u, -l, axis=1), axis=1) for l in range(ORDER + 1)], axis=1)
        else:
            r = np.stack([np.sum(u[:, :N - l] * u[:, l:], axis=1) for l in range(ORDER + 1)], axis=1)
        a, fail = levinson(r, order)
    else:
        # the DFT sum in extended precision (where the platform has it): band-limited speech leaves bins 1e-8 of the frame's
        # norm, whose logarithm magnifies the rounding of a float64 sum of N terms beyond what the two forms may differ by
        LD = np.longdouble
        th = 2.0 * np.arccos(LD(-1.0)) * (np.outer(np.arange(N), np.arange(nbin)) % NFFT).astype(LD) / NFFT
        ul = u.astype(LD)
        X = np.sqrt((ul @ np.cos(th)) ** 2 + (ul @ np.sin(th)) ** 2).astype(np.float64)
        ell = np.log(np.maximum(X, FLOOR))
        full = np.concatenate([ell, ell[:, NFFT // 2 - 1:0:-1]], axis=1)
        c = np.fft.ifft(full, axis=1).real[:, :NQ]
        B = X @ mel_matrix_interp(fs, NFFT).T
        r = np.array([np.correlate(f, f, "full")[N - 1:N + ORDER] for f in u]).reshape(nfr, ORDER + 1)
        a, fail = lpc_solve(r, order)
    if order < ORDER:
        a = np.concatenate([a, np.zeros((nfr, ORDER - order))], axis=1)
    return dict(nfr=nfr, n=n, P=float(np.sum(x * x)), X=X, c=c, B=B, r=r, a=a, fail=fail)


def quad(a, r, form="explicit"):
    """Q(a, r) = sum_i sum_j a[i] a[j] r[|i - j|] per frame: a, r [T, 13] -> [T]"""
    n = a.shape[1]
    if form == "explicit":
        q = np.zeros(a.shape[0])
        for i in range(n):
            row = np.zeros(a.shape[0])
            for j in range(n):
                row = row + a[:, j] * r[:, abs(i - j)]
            q = q + a[:, i] * row
        return q
    i = np.arange(n)
    return np.array([a[t] @ r[t][np.abs(i[:, None] - i[None, :])] @ a[t] for t in range(a.shape[0])])


def median(v, upper=False):
    v = np.sort(np.asarray(v, dtype=np.float64))
    K = v.shape[0]
    if K == 0:
        return np.nan
    if K % 2:
        return float(v[(K - 1) // 2])
    return float(v[K // 2]) if upper else float((v[K // 2 - 1] + v[K // 2]) / 2.0)


def pair(fx, fy, form="explicit", **faults):
    """the features of the reference x and of the estimate y -> dict: the six figures, frames, K, K_llr, valid, and the values
    of every frame cd_t / llr_t / fw_t [nfr] (NaN where the frame is not counted)"""
    nfr = fx["nfr"]
    used = fx["r"][:, 0] > 0
    K = int(np.sum(used))
    out = dict(frames=nfr, K=K, K_llr=0, valid=bool(K >= 1 and fx["P"] > 0), cd_t=np.full(nfr, np.nan),
               llr_t=np.full(nfr, np.nan), fw_t=np.full(nfr, np.nan))
    for key in FIGURES:
        out[key] = np.nan
    if not out["valid"]:
        return out
    with np.errstate(all="ignore"):
        d = fx["c"] - fy["c"]
        dbar = np.zeros(NQ) if faults.get("no_mean_norm") else d[used].mean(axis=0)
        dd = d - dbar[None, :]
        two = 1.0 if faults.get("no_factor2") else 2.0
        cd = (10.0 / np.log(10.0)) * np.sqrt(dd[:, 0] ** 2 + two * np.sum(dd[:, 1:] ** 2, axis=1))
        out["cd_t"] = np.where(used, np.minimum(cd, CD_CAP), np.nan)
        qy, qx = quad(fy["a"], fx["r"], form), quad(fx["a"], fx["r"], form)
        counts = used & ~fx["fail"] & ~fy["fail"] & (qy > 0) & (qx > 0)
        llr = np.clip(np.log(np.where(counts, qy, 1.0) / np.where(counts, qx, 1.0)), 0.0, LLR_CAP)
        out["llr_t"] = np.where(counts, llr, np.nan)
        gx = np.sqrt(fx["n"] / fx["P"]) if fx["P"] > 0 else 0.0
        gy = np.sqrt(fy["n"] / fy["P"]) if fy["P"] > 0 else 0.0
        if faults.get("no_gain"):
            gx = gy = 1.0
        Xb, Yb = gx * fx["B"], gy * fy["B"]
        W = Xb ** 0.2
        den = (Xb - Yb) ** 2
        snr = np.where(den == 0, SNR_HI, np.clip(10.0 * np.log10(Xb * Xb / np.where(den == 0, 1.0, den)), SNR_LO, SNR_HI))
        out["fw_t"] = np.where(used, np.sum(W * snr, axis=1) / np.sum(W, axis=1), np.nan)
    up = bool(faults.get("upper_median"))
    out["K_llr"] = int(np.sum(counts))
    out["cd"], out["cd_median"] = float(np.mean(out["cd_t"][used])), median(out["cd_t"][used], up)
    out["fwsegsnr"], out["fwsegsnr_median"] = float(np.mean(out["fw_t"][used])), median(out["fw_t"][used], up)
    if out["K_llr"] > 0:
        out["llr"], out["llr_median"] = float(np.mean(out["llr_t"][counts])), median(out["llr_t"][counts], up)
    return out


def explicit(x, y, fs, **faults):
    """x the clean reference, y the estimate (int16 or float), both [n] at rate fs -> the dict of :func:`pair`"""
    return pair(features(x, fs, "explicit", **faults), features(y, fs, "explicit", **faults), "explicit", **faults)


def direct(x, y, fs):
    return pair(features(x, fs, "direct"), features(y, fs, "direct"), "direct")


def best_perm(cd):
    """cd [S estimates, S references] -> p, p[j] = the estimate of reference j: the first permutation in itertools order with
    the least sum_j cd[p[j], j]; a non-finite term makes a permutation lose"""
    cd = np.asarray(cd, dtype=np.float64)
    S = cd.shape[0]
    best, vbest = None, None
    for p in itertools.permutations(range(S)):
        terms = [-cd[p[j], j] for j in range(S)]
        v = float(sum(terms)) if all(np.isfinite(t) for t in terms) else -np.inf
        if best is None or v > vbest:
            best, vbest = list(p), v
    return best


def recording(est, clean, mix, fs, form="explicit", **faults):
    """est [S, L], clean [S, L], mix [L] or None -> what ``score.reverb_waves`` reports, as a dict of arrays, plus ``matrix``
    [S (+ 1), S, 6] (the figures of every pair, the mixture last), ``counts`` [S (+ 1), S, 3] = (frames, K, K_llr) and
    ``frame_values`` [S (+ 1), S, 3, frames] (the CD, LLR and fwSegSNR of every frame)"""
    est, clean = np.asarray(est), np.asarray(clean)
    S = clean.shape[0]
    fr = [features(clean[j], fs, form, **faults) for j in range(S)]
    fe = [features(est[i], fs, form, **faults) for i in range(S)]
    if mix is not None:
        fe.append(features(np.asarray(mix), fs, form, **faults))
    E = len(fe)
    pairs = [[pair(fr[j], fe[i], form, **faults) for j in range(S)] for i in range(E)]
    matrix = np.array([[[pairs[i][j][k] for k in FIGURES] for j in range(S)] for i in range(E)])
    counts = np.array([[[pairs[i][j][k] for k in ("frames", "K", "K_llr")] for j in range(S)] for i in range(E)])
    frame_values = np.array([[[pairs[i][j][k] for k in ("cd_t", "llr_t", "fw_t")] for j in range(S)] for i in range(E)])
    p = best_perm(matrix[:S, :, 0])
    idx = np.arange(S)
    out = dict(perm_best=p, frames=counts[idx, idx, 0], frames_used=counts[idx, idx, 1], frames_llr=counts[idx, idx, 2],
               valid=np.array([pairs[j][j]["valid"] for j in range(S)]), matrix=matrix, counts=counts, frame_values=frame_values)
    for k, key in enumerate(FIGURES):
        out[key] = matrix[idx, idx, k]
        out[key + "_best"] = np.array([matrix[p[j], j, k] for j in range(S)])
        out[key + "_mix"] = matrix[S, :, k] if mix is not None else None
        out[key + "_i"] = out[key + "_best"] - out[key + "_mix"] if mix is not None else None
    return out


def deviation(a, b):
    """the largest |a - b| over the figures, the pair matrices and the values of every frame of two :func:`recording` dicts
    (NaN against NaN counts as equal, NaN against a number as infinite)"""
    worst = 0.0
    for key in ("matrix", "frame_values"):
        x, y = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        if x.shape != y.shape or np.any(np.isnan(x) != np.isnan(y)):
            return np.inf
        d = np.abs(x - y)
        if d.size and np.any(~np.isnan(d)):
            worst = max(worst, float(np.nanmax(d)))
    return worst


_inputs, _oracle = {}, {}


def inputs():
    """{tag: (est, clean, mix, fs)}: the real speech and the six synthetic cases, built once"""
    if not _inputs:
        from conftest import golden
        _inputs["golden"] = golden_case(golden("g16_stoi.npz"))
        for k in range(len(CASES)):
            _inputs[f"case{k}"] = synthetic(k)
    return _inputs


def oracle(tag):
    """:func:`recording` in the explicit form of one of :func:`inputs`, computed once and shared; nobody writes into it"""
    if tag not in _oracle:
        _oracle[tag] = recording(*inputs()[tag])
    return _oracle[tag]
