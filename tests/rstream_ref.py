"""NumPy float64 restatement of the streaming polyphase resampler (C ABI misonet_resample_stream): the count
formulas, the carried tail, the walk over "carried tail ++ block" in the coordinates of the block, the flush -- and, behind
``fault=``, the mistakes such code invites.  The offline definition and its restatement are tests/resample_ref.py's.

A stream has seen N samples.  Output m is complete once its last input floor((m q + Lh) / p) has arrived:
e(N) = 0 where N p - 1 - Lh < 0, else floor((N p - 1 - Lh) / q) + 1.  A call emits [e(N), e(N + n_new)), a flushing call
[e(N), ceil((N + n_new) p / q)).  The next output needs at most the last C = floor(2 Lh / p) samples.
"""
import numpy as np

import resample_ref as R

FAULTS = ("carry_short", "carry_stall", "phase_from_block", "emitted_off_by_one", "flush_feeds_zeros", "i16_scale_per_term")


def carry(p, q):
    return 2 * R.half_len(p, q) // p


def emitted(N, p, q, fault=None):
    a = N * p - 1 - R.half_len(p, q)
    if a < 0:
        return 0
    if fault == "emitted_off_by_one":
        return -(-a // q)                      # ceil(a / q): one short exactly where a = 0 (mod q)
    return a // q + 1


def outputs(n_seen, n_new, flush, p, q):
    """what a call emits; -1 for the arguments the library refuses"""
    if n_seen < 0 or n_new < 0 or n_new > (1 << 28) or n_seen > (1 << 50) or (n_new == 0 and not flush):
        return -1
    E = R.out_len(n_seen + n_new, p, q) if flush else emitted(n_seen + n_new, p, q)
    return E - emitted(n_seen, p, q)


def latency(p, q):
    """input samples between a sample's arrival and the output at its own instant"""
    return R.half_len(p, q) / p


def cut(n, pieces):
    """the block lengths of a stream of n samples: ``pieces`` cycled, the last one shortened"""
    out, k = [], 0
    while n > 0:
        c = min(int(pieces[k % len(pieces)]), n)
        out.append(c)
        n -= c
        k += 1
    return out


def _call(tail, blk, n_out, D, p, q, Lh, g, scale_terms):
    """n_out outputs from the tail [C, M] and the block [n_new, M]: output i is sum_jr x[jr] g[D + i q - jr p + Lh], jr ascending
    over [-C, n_new) with the tap index in [0, 2 Lh]; jr < 0 reads the tail"""
    C, n_new = tail.shape[0], blk.shape[0]
    buf = np.concatenate([tail, blk], axis=0)
    i = np.arange(n_out, dtype=np.int64)
    c = D + i * q
    j_lo = np.maximum(-C, -((Lh - c) // p))
    j_hi = np.minimum(n_new - 1, (c + Lh) // p)
    acc = np.zeros((n_out, blk.shape[1]))
    steps = int((j_hi - j_lo).max()) + 1 if n_out else 0
    for s in range(max(steps, 0)):
        j = j_lo + s
        t = c - j * p + Lh
        live = (j <= j_hi) & (t >= 0) & (t < g.size)
        jj, tt = np.where(live, j + C, 0), np.where(live, t, 0)
        x = buf[jj] * (1.0 / 32767.0) if scale_terms else buf[jj]
        acc = acc + np.where(live[:, None], x * g[tt][:, None], 0.0)
    return acc


def stream(x, p, q, cuts, g=None, fault=None, flush_with_block=True, in_i16=False):
    """x [n] or [n, M] (float, or the integer values of int16 samples with ``in_i16``) fed in blocks of ``cuts`` (see ``cut``),
    the flush carrying the last block or none -> float64 [ceil(n p / q)(, M)], the outputs of all calls concatenated"""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    if one:
        x = x[:, None]
    n, M = x.shape
    Lh, C = R.half_len(p, q), carry(p, q)
    g = R.firwin_taps(p, q) if g is None else np.asarray(g, dtype=np.float64)
    tail = np.zeros((C, M))
    keep = C - 1 if fault == "carry_short" else C
    N, out = 0, []
    blocks = cut(n, cuts)
    calls = [(b, False) for b in blocks]
    if flush_with_block and calls:
        calls[-1] = (calls[-1][0], True)
    else:
        calls.append((0, True))
    ef = fault if fault == "emitted_off_by_one" else None
    for n_new, flush in calls:
        blk = x[N:N + n_new]
        e0 = emitted(N, p, q, ef)                                # the fault: where a call starts, not where the last one ended
        if flush and fault == "flush_feeds_zeros":               # the end as zero SAMPLES, not cut at the offline length
            Z = -(-(Lh + 1 + q) // p)
            blk = np.concatenate([blk, np.zeros((Z, M))], axis=0)
            E = emitted(N + n_new + Z, p, q)
        else:
            E = R.out_len(N + n_new, p, q) if flush else emitted(N + n_new, p, q)
        D = e0 * q - N * p
        if fault == "phase_from_block":
            D = emitted(n_new, p, q) * q - n_new * p
        y = _call(tail, blk, E - e0, D, p, q, Lh, g, in_i16 and fault == "i16_scale_per_term")
        if in_i16 and fault != "i16_scale_per_term":
            y = y * (1.0 / 32767.0)                                # scaled once, after the sum
        out.append(y)
        if not (fault == "carry_stall" and E == e0):
            both = np.concatenate([tail, x[N:N + n_new]], axis=0)
            tail = both[both.shape[0] - C:]
            if keep < C and C > 0:
                tail = tail.copy()
                tail[:C - keep] = 0.0
        N += n_new
    y = np.concatenate(out, axis=0) if out else np.zeros((0, M))
    return y[:, 0] if one else y
