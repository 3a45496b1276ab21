"""NumPy restatement of the polyphase resampler (csrc/resample.hip) in the kernel's summation order, the
float64 oracle (``scipy.signal.resample_poly`` itself), the generators of the tests' inputs, the bars and the planted faults.

Definition, for p / q = fs_out / fs_in in lowest terms:  Lh = 10 max(p, q);  g = p firwin(2 Lh + 1, 1 / max(p, q),
window=("kaiser", 5.0));  y[m] = sum_j x[j] g[m q - j p + Lh] with j ascending over 0 <= j < n and the tap index in [0, 2 Lh];
ceil(n p / q) outputs;  zeros outside the signal;  every channel on its own.  p = q = 1: Lh = 0, g = [1].

The bar of a float32 result (``bar``): e0 = rel-L2 of float32(ref64) against ref64, the error of rounding the exact answer once;
the device computes a float64 sum and rounds it once, so it sits at e0, and 2 e0 only absorbs the ties that the float64 sum's own
error (1e-16 relative, against float32's 6e-8) moves across a rounding boundary.
"""
import math

import numpy as np

# p / q of the tests, as (fs_in, fs_out) pairs that reduce to them
RATIOS = {"1/1": (8000, 8000), "1/2": (16000, 8000), "2/1": (8000, 16000), "1/3": (48000, 16000), "3/1": (16000, 48000),
          "160/441": (44100, 16000), "441/160": (16000, 44100), "147/160": (48000, 44100), "80/441": (44100, 8000)}
CHANNELS = (1, 2, 6, 7, 8)
FAULTS = ("phase", "centre", "last_tap", "swap_pq", "j_lo_short", "j_hi_short", "neighbour_channel", "f32_acc")


def pq(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def half_len(p, q):
    return 0 if p == q == 1 else 10 * max(p, q)


def out_len(n, p, q):
    return -(-n * p // q)


def firwin_taps(p, q):
    """g of the definition, from SciPy's own firwin"""
    from scipy.signal import firwin
    if p == q == 1:
        return np.ones(1)
    Lh = half_len(p, q)
    return firwin(2 * Lh + 1, 1.0 / max(p, q), window=("kaiser", 5.0)) * p


def oracle(x, p, q):
    """scipy.signal.resample_poly along axis 0 in float64 (its 1 / 1 is a copy)"""
    from scipy.signal import resample_poly
    return resample_poly(np.asarray(x, dtype=np.float64), p, q, axis=0)


def restate(x, p, q, g=None, fault=None):
    """x float [n] or [n, M] -> float64 of the same rank with ceil(n p / q) samples: the sum of the definition, term after term
    with j ascending (all outputs advance together, each through its own j).  ``fault``: one of FAULTS."""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    if one:
        x = x[:, None]
    n, M = x.shape
    if fault == "swap_pq":
        p, q = q, p
    Lh = half_len(p, q)
    g = firwin_taps(p, q) if g is None else np.asarray(g, dtype=np.float64)
    if fault == "last_tap":
        g = g.copy()
        g[-1] = 0.0
    n_out = out_len(n, p, q)
    c = (Lh - 1) if (fault == "centre" and Lh > 0) else Lh
    m = np.arange(n_out, dtype=np.int64)
    j_lo = np.maximum(0, -((c - m * q) // p))                   # ceil((m q - c) / p)
    j_hi = np.minimum(n - 1, (m * q + c) // p)
    if fault == "j_lo_short":
        j_lo = j_lo + 1
    if fault == "j_hi_short":
        j_hi = j_hi - 1
    xs = np.roll(x, 1, axis=1) if fault == "neighbour_channel" else x
    acc_t = np.float32 if fault == "f32_acc" else np.float64
    acc = np.zeros((n_out, M), dtype=acc_t)
    steps = int((j_hi - j_lo).max()) + 1 if n_out else 0
    for s in range(steps):
        j = j_lo + s
        live = j <= j_hi
        t = m * q - j * p + c + (1 if fault == "phase" else 0)
        live &= (t >= 0) & (t < g.size)
        jj, tt = np.where(live, j, 0), np.where(live, t, 0)
        term = xs[jj].astype(acc_t) * g[tt].astype(acc_t)[:, None]
        acc = acc + np.where(live[:, None], term, acc_t(0))
    y = acc.astype(np.float64)
    return y[:, 0] if one else y


def support(j, n, p, q):
    """the outputs whose sum contains input sample j: m with 0 <= m q - j p + Lh <= 2 Lh, below ceil(n p / q)"""
    Lh = half_len(p, q)
    m = np.arange(out_len(n, p, q), dtype=np.int64)
    t = m * q - j * p + Lh
    return (t >= 0) & (t <= 2 * Lh)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / d) if d > 0 else float(np.linalg.norm(a - b))


def e0(ref64):
    """(rel-L2 of float32(ref64) against ref64 over the whole tensor, the largest such figure of one channel)"""
    r = np.asarray(ref64, dtype=np.float64).reshape(-1, np.shape(ref64)[-1])
    r32 = r.astype(np.float32)
    return rel(r32, r), max(rel(r32[:, c], r[:, c]) for c in range(r.shape[1]))


def figures(got, ref64):
    """(whole-tensor rel-L2, worst-channel rel-L2) of a float32 result [.., M] against ref64"""
    a = np.asarray(got, dtype=np.float64).reshape(-1, np.shape(ref64)[-1])
    r = np.asarray(ref64, dtype=np.float64).reshape(a.shape)
    return rel(a, r), max(rel(a[:, c], r[:, c]) for c in range(r.shape[1]))


def within_bar(got, ref64):
    """the bar of the module text: both figures within 2 e0.  -> (passed, whole, worst channel, e0 whole, e0 worst channel)"""
    w, c = figures(got, ref64)
    ew, ec = e0(ref64)
    return (w <= 2 * ew and c <= 2 * ec), w, c, ew, ec


def noise(n, M, seed, scale=0.3, dtype=np.float32):
    """white noise at `scale` of full scale, [n, M]; int16: the same x 32767, rounded"""
    x = np.random.default_rng(seed).standard_normal((n, M)) * scale / 3.0          # 3 sigma at `scale`
    x = np.clip(x, -1.0, 1.0)
    if dtype == np.int16:
        return np.rint(x * 32767.0).astype(np.int16)
    return x.astype(np.float32)


def lengths(p, q, tile):
    """the input lengths of one ratio: 1, 2, one below Lh / q; n p mod q in {0, 1, q - 1}; and the smallest n whose output
    count reaches tile - 1, tile, tile + 1 and 2 tile + 1 (with p > 1 not every count exists: the next one that does)"""
    Lh = half_len(p, q)
    ns = {1, 2, max(1, Lh // q - 1)}
    for r in {0, 1 % q, q - 1}:
        ns.add(next(n for n in range(40, 40 + 2 * q + 2) if (n * p) % q == r))
    for want in (tile - 1, tile, tile + 1, 2 * tile + 1):
        ns.add(max(1, -(-want * q // p)))
    return sorted(ns)


def rint_i16(y64):
    """float64 waveform -> (rint(y x 32767) saturated to int16 as int64, the mask of values further than 1e-6 from a half-integer)"""
    v = np.asarray(y64, dtype=np.float64) * 32767.0
    frac = np.abs(v - np.floor(v) - 0.5)
    return np.clip(np.rint(v), -32768, 32767).astype(np.int64), frac > 1e-6
