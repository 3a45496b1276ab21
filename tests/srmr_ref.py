"""The speech-to-reverberation modulation energy ratio restated in NumPy / SciPy, in two independent forms,
plus the inputs shared by tests/test_srmr.py and tests/test_gpu_srmr.py.

  * :func:`measure` -- the oracle, form (a).  ``scipy.signal.lfilter`` for the four gammatone sections and the modulation
    filters, ``scipy.signal.hilbert(y, N=P)`` for the envelope, every frame cut out and weighted on its own.
  * :func:`measure_ld` -- form (b).  Every recurrence in ``np.longdouble``, stepped in one loop over the samples with all bands
    as a vector; the envelope from ``numpy.fft`` on the padded signal with the one-sided mask applied by hand; the frame
    energies from a cumulative sum per window phase.  :func:`d64` is the distance between the two on an input: how much of a
    deviation is the conditioning of the filters in float64 (the 4 Hz modulation filter has its poles next to z = 1).

An int16 sample q stands for q / 32767.  Every name in ``FAULTS`` plants one fault into form (a): tests/test_srmr.py shows that
the ceiling the GPU test asserts rejects each of them.  No SRMR toolbox was available: nothing here was compared against one.
"""
import cmath
import functools
import math

import numpy as np
import scipy.signal

RATES = (8000, 16000)
NCH, NMOD = 23, 8
EARQ, MINBW = 9.26449, 24.7
CHUNK = 4096                 # where the chunk faults put their seams; the GPU test takes the device's own value for its lengths

# device - oracle (a) over every input of tests/test_gpu_srmr.py (Ebar relative to its maximum, SRMR and BW relative): ten times
# the largest deviation measured on an MI355X, rounded up to a power of ten (the measured figures are in the GPU test's
# docstring).  The issue's condition on it: at most 1 / 100 of the smallest shift of a planted fault.
DEV_CEIL = 1e-10

FAULTS = ("periodic_window", "no_1019", "no_gain_band", "circular_hilbert", "squared_env", "seam_zero", "late_transition",
          "drop_last", "k_plus_one", "from_channel_0", "q1", "linear_centres", "f32_env")
# "hop floor for ceil" is not among them: 0.064 fs and 0.256 fs are integers at both rates, so the two agree everywhere


# ---- the design --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def design(fs, no_1019=False, q1=False, linear_centres=False):
    """the filters, from ``math`` scalars in the order the definition writes them: the coefficients of the 4 Hz modulation filter
    decide its response to some 1e-10 per unit in their last place, so the library and the oracle must round them alike"""
    if fs not in RATES:
        raise ValueError(f"SRMR is defined here for fs = 8000 or 16000 Hz (got {fs})")
    pi = math.pi
    c = EARQ * MINBW
    T = 1.0 / fs
    rr = (math.sqrt(3.0 + math.pow(2.0, 1.5)), -math.sqrt(3.0 + math.pow(2.0, 1.5)),
          math.sqrt(3.0 - math.pow(2.0, 1.5)), -math.sqrt(3.0 - math.pow(2.0, 1.5)))
    cf, erb, gain = np.zeros(NCH), np.zeros(NCH), np.zeros(NCH)
    a, b = np.zeros((NCH, 3)), np.zeros((NCH, 4, 3))
    for j in range(NCH):
        i = NCH - j                                                  # ERBSpace descends; channel j ascends
        cf[j] = -c + math.exp(i * (math.log(125.0 + c) - math.log(0.5 * fs + c)) / NCH) * (0.5 * fs + c)
        erb[j] = cf[j] / EARQ + MINBW
        Bw = (1.0 if no_1019 else 1.019) * 2.0 * pi * erb[j]
        c1, s1, e = math.cos(2.0 * pi * cf[j] * T), math.sin(2.0 * pi * cf[j] * T), math.exp(-Bw * T)
        a[j] = (1.0, -2.0 * c1 * e, e * e)
        zi = cmath.exp(complex(0.0, -2.0 * pi * cf[j] * T))
        H = complex(1.0, 0.0)
        for s in range(4):
            b[j, s] = (T, -(2.0 * T * c1 * e + 2.0 * rr[s] * T * s1 * e) / 2.0, 0.0)
            H *= (b[j, s, 0] + b[j, s, 1] * zi) / (1.0 + a[j, 1] * zi + a[j, 2] * zi * zi)
        gain[j] = 1.0 / abs(H)
    fk, ll = np.zeros(NMOD), np.zeros(NMOD)
    mb, ma = np.zeros((NMOD, 3)), np.zeros((NMOD, 3))
    Q = 1.0 if q1 else 2.0
    for k in range(NMOD):
        fk[k] = 4.0 + k * (128.0 - 4.0) / 7.0 if linear_centres else 4.0 * math.pow(32.0, k / 7.0)
        W = math.tan(pi * fk[k] / fs)
        beta = W / Q
        mb[k] = (beta, 0.0, -beta)
        ma[k] = (1.0 + beta + W * W, 2.0 * W * W - 2.0, 1.0 - beta + W * W)
        ll[k] = fk[k] - beta * fs / (2.0 * pi)
    Nw, Hw = (256 * fs + 999) // 1000, (64 * fs + 999) // 1000      # ceil(0.256 fs), ceil(0.064 fs)
    assert Nw == math.ceil(0.256 * fs) and Hw == math.ceil(0.064 * fs) and Nw == 4 * Hw
    win = np.array([0.54 - 0.46 * math.cos(2.0 * pi * i / (Nw - 1)) for i in range(Nw)])
    return dict(fs=fs, cf=cf, erb=erb, a=a, b=b, gain=gain, mb=mb, ma=ma, fk=fk, ll=ll, Nw=Nw, Hw=Hw, win=win,
                win_periodic=0.54 - 0.46 * np.cos(2 * np.pi * np.arange(Nw) / Nw))


def frames_of(n, fs):
    d = design(fs)
    return 1 + (n - d["Nw"]) // d["Hw"] if n >= d["Nw"] else 0


def as_float64(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32767.0
    return x.astype(np.float32).astype(np.float64)


def _lfilter_chunked(b, a, x, fault):
    """lfilter run chunk by chunk with the state carried as the scan carries it (zero-state response + transition), with a
    fault planted: ``seam_zero`` starts chunk 1 from zero state, ``late_transition`` applies A^C to the state of the chunk
    before the one it belongs to"""
    n, C = x.shape[0], CHUNK
    zero = np.zeros(2)
    y = np.empty(n)
    states = [zero]                                                  # the true state chunk c starts from
    for c in range((n + C - 1) // C):
        seg = x[c * C:(c + 1) * C]
        s = states[c]
        if fault == "seam_zero" and c == 1:
            s = zero
        y[c * C:(c + 1) * C], _ = scipy.signal.lfilter(b, a, seg, zi=s)
        if seg.shape[0] == C:
            _, f = scipy.signal.lfilter(b, a, seg, zi=zero)
            src = states[c - 1] if (fault == "late_transition" and c >= 1) else states[c]
            _, hom = scipy.signal.lfilter(b, a, np.zeros(C), zi=src)
            states.append(hom + f)
    return y


def finish(E, nfr, d, fault=None):
    """steps 6 and 7 from the mean energies E [23, 8]"""
    res = dict(energy=E, frames=int(nfr), valid=False, srmr=np.nan, k_star=0, bw=np.nan, run=None, j_star=-1)
    if nfr < 1:
        res["energy"] = np.full((NCH, NMOD), np.nan)
        return res
    A = np.array([sum(E[j, k] for k in range(NMOD)) for j in range(NCH)])
    tot = 0.0
    for j in range(NCH):
        tot += A[j]
    if not tot > 0.0:
        return res
    order = range(NCH) if fault == "from_channel_0" else range(NCH - 1, -1, -1)
    run, js, runs = 0.0, 0, []
    for j in order:
        run += 100.0 * A[j] / tot
        runs.append(run)
        if run > 90.0:
            js = j
            break
    bw = d["erb"][js]
    K = 5 + int(bw >= d["ll"][5]) + int(bw >= d["ll"][6]) + int(bw >= d["ll"][7])
    if fault == "k_plus_one":
        K += 1
    num = den = 0.0
    for j in range(NCH):
        for k in range(4):
            num += E[j, k]
        for k in range(4, min(K, NMOD)):
            den += E[j, k]
    res.update(valid=True, srmr=num / den, k_star=K, bw=float(bw), j_star=js, run=runs[-2:] if len(runs) > 1 else [0.0] + runs)
    return res


def measure(x, fs, fault=None):
    """form (a): dict(energy [23, 8], srmr, k_star, bw, frames, valid, run = the running sums before and at j*)"""
    assert fault is None or fault in FAULTS
    d = design(fs, no_1019=fault == "no_1019", q1=fault == "q1", linear_centres=fault == "linear_centres")
    x = as_float64(x)
    n = x.shape[0]
    Nw, Hw = d["Nw"], d["Hw"]
    nfr = frames_of(n, fs)
    if nfr < 1:
        return finish(None, 0, d)
    if fault == "drop_last":
        nfr -= 1
    P = 1 << int(n - 1).bit_length()
    win = d["win_periodic"] if fault == "periodic_window" else d["win"]
    E = np.zeros((NCH, NMOD))
    chunked = fault in ("seam_zero", "late_transition")
    for j in range(NCH):
        y = x * (1.0 if (fault == "no_gain_band" and j == 11) else d["gain"][j])
        for s in range(4):
            y = _lfilter_chunked(d["b"][j, s], d["a"][j], y, fault) if chunked else scipy.signal.lfilter(d["b"][j, s], d["a"][j], y)
        env = np.abs(scipy.signal.hilbert(y) if fault == "circular_hilbert" else scipy.signal.hilbert(y, N=P)[:n])
        if fault == "squared_env":
            env = env * env
        if fault == "f32_env":
            env = env.astype(np.float32).astype(np.float64)
        for k in range(NMOD):
            m = _lfilter_chunked(d["mb"][k], d["ma"][k], env, fault) if chunked else scipy.signal.lfilter(d["mb"][k], d["ma"][k], env)
            fr = np.lib.stride_tricks.sliding_window_view(m, Nw)[::Hw][:nfr]
            E[j, k] = np.mean(np.sum((fr * win) ** 2, axis=1)) if nfr else np.nan
    return finish(E, nfr, d, fault)


def _biquad_ld(b, a, x):
    """x [n, V] through V biquads b, a [V, 3] (a[:, 0] = 1) in longdouble, transposed direct form II, one loop over the samples"""
    b, a = b.astype(np.longdouble), a.astype(np.longdouble)
    z0 = np.zeros(b.shape[0], np.longdouble)
    z1 = z0.copy()
    y = np.empty(x.shape, np.longdouble)
    for i in range(x.shape[0]):
        xi = x[i]
        yi = z0 + b[:, 0] * xi
        z0 = z1 + b[:, 1] * xi - a[:, 1] * yi
        z1 = b[:, 2] * xi - a[:, 2] * yi
        y[i] = yi
    return y


def measure_ld(x, fs):
    """form (b)"""
    d = design(fs)
    x = as_float64(x)
    n = x.shape[0]
    Nw, Hw = d["Nw"], d["Hw"]
    nfr = frames_of(n, fs)
    if nfr < 1:
        return finish(None, 0, d)
    y = x.astype(np.longdouble)[:, None] * d["gain"].astype(np.longdouble)[None, :]
    for s in range(4):
        y = _biquad_ld(d["b"][:, s], d["a"], y)
    P = 1 << int(n - 1).bit_length()
    pad = np.zeros((P, NCH))
    pad[:n] = y.astype(np.float64)
    Y = np.fft.fft(pad, axis=0)
    mask = np.zeros(P)
    mask[0] = 1.0
    if P > 1:
        mask[P // 2] = 1.0
        mask[1:P // 2] = 2.0
    env = np.abs(np.fft.ifft(Y * mask[:, None], axis=0))[:n]
    ma = (d["ma"] / d["ma"][:, :1]).astype(np.longdouble)
    mb = (d["mb"].astype(np.longdouble) / d["ma"][:, :1].astype(np.longdouble))
    E = np.zeros((NCH, NMOD))
    w2 = (d["win"].astype(np.longdouble)) ** 2
    for j in range(NCH):
        m = _biquad_ld(mb, ma, np.repeat(env[:, j:j + 1].astype(np.longdouble), NMOD, axis=1))
        m2 = m * m
        tot = np.zeros(NMOD, np.longdouble)
        for t in range(nfr):
            tot += (m2[t * Hw:t * Hw + Nw] * w2[:, None]).sum(axis=0)
        E[j] = (tot / nfr).astype(np.float64)
    return finish(E, nfr, d)


def deviation(a, b):
    """what the GPU test compares between two results: Ebar relative to the maximum of a, SRMR and BW relative; inf where
    K*, the frames or the validity differ"""
    if a["frames"] != b["frames"] or a["valid"] != b["valid"] or a["k_star"] != b["k_star"]:
        return np.inf
    if not a["valid"]:
        return 0.0
    return float(max(np.max(np.abs(a["energy"] - b["energy"])) / np.max(a["energy"]), abs(a["srmr"] - b["srmr"]) / abs(a["srmr"]),
                     abs(a["bw"] - b["bw"]) / a["bw"]))


def d64(x, fs):
    return deviation(measure(x, fs), measure_ld(x, fs))


def margin_ok(res, fs):
    """the condition on an input of a comparison: the running sum at j* and the one before it at least 0.25 points from 90, BW
    at least 1 % from every ll_k"""
    d = design(fs)
    return bool(res["valid"] and all(abs(r - 90.0) >= 0.25 for r in res["run"])
                and np.all(np.abs(res["bw"] - d["ll"]) >= 0.01 * res["bw"]))


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
def synthetic(fs, n, t60=0.0, seed=0, level=0.25):
    """AR(2) noise under a 3.7 Hz envelope with gated pauses, convolved with a decaying-noise response of that T60 (0: dry),
    float32 [n] with its peak at ``level``"""
    rng = np.random.default_rng(1000 * seed + int(10 * t60) + (7 if fs == 8000 else 0))
    m = n + int(0.1 * fs)
    e = rng.standard_normal(m)
    r, th = 0.97, 2 * np.pi * 900.0 / fs
    s = scipy.signal.lfilter([1.0], [1.0, -2 * r * np.cos(th), r * r], e)
    t = np.arange(m) / fs
    env = 0.5 * (1.0 + np.sin(2 * np.pi * 3.7 * t + rng.uniform(0, 2 * np.pi)))
    gate = (np.sin(2 * np.pi * 0.8 * t + rng.uniform(0, 2 * np.pi)) > -0.6).astype(np.float64)
    s = s * env * gate + 1e-3 * rng.standard_normal(m)
    if t60 > 0:
        L = int(t60 * fs)
        h = rng.standard_normal(L) * np.exp(-6.9078 * np.arange(L) / (t60 * fs))
        h[0] = 1.0
        s = scipy.signal.fftconvolve(s, h)[:m]
    s = s[m - n:]
    return (level * s / np.max(np.abs(s))).astype(np.float32)


def to_i16(x):
    return np.clip(np.round(np.asarray(x, np.float64) * 32767.0), -32768, 32767).astype(np.int16)


GOLDEN_START = 3600      # as tests/reverb_ref.py: the first reference of the golden recording starts with digital silence


def golden_signals(g):
    """the real speech of tests/golden/g16_stoi.npz (8 kHz): (signals float32 [2, L] = the two estimates, mix float32 [L], fs)"""
    est = (g["est_q"].astype(np.float64) / float(1 << 23)).astype(np.float32)[:, GOLDEN_START:]
    clean = g["clean"][:, GOLDEN_START:]
    return np.ascontiguousarray(est), (clean[0] + clean[1]).astype(np.float32), int(g["fs"])


GOLDEN_SLICE = (8000, 32000)     # where the two estimates and the mixture of the golden all keep the margin (margin_ok)
T60S = (0.0, 0.3, 0.7, 1.2)
# the seed of synthetic() for an input (fs, n, T60, int16): 1 unless the margin condition asked for another (picked on the oracle
# alone; tests/test_srmr.py asserts the condition on every input below)
SEEDS = {(8000, 2560, 1.2, False): 2, (16000, 48000, 0.7, True): 2}
# the recordings of the GPU test: (fs, n, the T60 of each signal, the T60 of the mixture or None, int16)
FAMILY = [(16000, 48000, (0.0, 0.3, 0.7), 1.2, True), (8000, 30011, (0.0, 0.7), 1.2, False), (16000, 20011, (0.3,), 1.2, True),
          (8000, 14001, (0.7,), None, False)]
LONG = (16000, 600000, 1.2)      # P = 2^20: the four-step route with both factors 1024
# where the planted faults are judged: three inputs of the GPU test, one of them longer than two chunks, one a single 8 kHz
# frame (the float32 rounding of the envelope averages out over many frames: it moves the long inputs by 1e-9 only)
FAULT_INPUTS = [(16000, 20011, 0.3, True), (8000, 14001, 0.7, False), (8000, 2048, 1.2, False)]


def edge_lengths(fs, C):
    """the lengths at which a mechanism changes, with the T60 each is given: the frame edges; at 16 kHz also the seams of the
    scan (chunks of C samples) and the sizes around one LDS pass of 4096 points (P = 4096 | 8192 | 16384)"""
    d = design(fs)
    Nw, Hw = d["Nw"], d["Hw"]
    ns = [Nw - 1, Nw, Nw + Hw - 1, Nw + Hw]
    if fs == 16000:
        ns += [C - 1, C, C + 1, 2 * C + 1, 3 * C, 4096, 4097, 8192, 8193]
    ns = sorted(set(ns))
    return [(n, T60S[i % 4]) for i, n in enumerate(ns)]


def signal(fs, n, t60, i16=False):
    x = synthetic(fs, n, t60, SEEDS.get((fs, n, t60, bool(i16)), 1))
    return to_i16(x) if i16 else x


@functools.lru_cache(maxsize=None)
def oracle_of(fs, n, t60, i16=False):
    """form (a) of signal(fs, n, t60, i16), computed once per process"""
    return measure(signal(fs, n, t60, i16), fs)


def mix_of(fs, n, t60):
    """the mixture of a family recording: float32 always"""
    return signal(fs, n, t60, False)
