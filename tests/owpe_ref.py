"""Float64 NumPy restatement of the online WPE of csrc/owpe.hip (include/misonet.h, "online WPE"), vectorised
over the bins.  The project's own definition in the RLS-WPE family (Yoshioka & Nakatani 2012; Caroselli et al. 2017; nara_wpe's
``online_wpe_step``); nara_wpe was not available and was not compared.

Per (item b, bin f), N = M taps.  State: P [N, N], G [N, M], the last delay + taps - 1 frames (complex64 as read), the powers of
the last ``context`` frames, n, fail.  ``reset``: P = init I, the rest 0.  Per new frame y:

    1. z[k M + m] = y[m, t - delay - k]                  (0 before the start of the stream)
    2. x = y - G^H z                                      (the output, rounded once to complex64)
    3. lambda = max(mean of p over the min(n, context) + 1 latest frames, this one included, power_floor), p = mean_m |y_m|^2
    4. u = P z;  d = alpha lambda + Re(z^H u);  k = u / d
    5. P <- (P - k u^H) / alpha                           (lower triangle computed, the upper its mirror: exactly Hermitian)
    6. G <- G + k x^H
    7. the frame enters the frame ring, p the power ring, n <- n + 1

A failing frame (a non-finite sample, or d not finite or not > 0): x = y, P and G stay, the frame enters the ring as zeros and p
as 0, fail |= 1, n advances.

The device tests compare against this file; ``FAULTS`` are the planted mistakes that tests/test_owpe.py shows the device
tests' bars reject, and ``fixed_room`` is the scene of the quality condition.
"""
import numpy as np

OUT_BAR = 2.4e-7            # one complex64 rounding of a float64 result (the bar of test_gpu_wpe.py)
STATE_FLOOR = 1e-12         # G and P: 100 x the restatement's own reversed-summation-order difference, never below this
FAULTS = ("z_late", "lambda_without_current", "p_not_divided", "k_zhp", "g_with_y", "float32_d")


class State:
    """the state of B x F bins; the rings in age order (index a - 1 = the frame a back)"""

    def __init__(self, B, M, F, taps=10, delay=3, context=0, alpha=0.999, power_floor=1e-10, init=1.0):
        self.B, self.M, self.F = B, M, F
        self.taps, self.delay, self.context = taps, delay, context
        self.alpha, self.power_floor, self.init = alpha, power_floor, init
        self.reset()

    def reset(self):
        B, M, F, N = self.B, self.M, self.F, self.M * self.taps
        self.P = np.zeros((B, F, N, N), np.complex128)
        self.P[:, :, np.arange(N), np.arange(N)] = self.init
        self.G = np.zeros((B, F, N, M), np.complex128)
        self.ring = np.zeros((B, F, self.delay + self.taps - 1 + 1, M), np.complex64)      # one more: the "z_late" fault
        self.pw = np.zeros((B, F, max(self.context, 1)), np.float64)
        self.n = np.zeros((B, F), np.int32)
        self.fail = np.zeros((B, F), np.int32)
        self.extra = None                    # the rings of companion signals (fixed_room's early and late parts)


def _matvec(P, z, reverse):
    """u = P z with the columns added in ascending (or descending) order of plain partial sums"""
    t = P * z[..., None, :]
    if reverse:
        t = t[..., ::-1]
    return np.add.reduce(np.ascontiguousarray(t), axis=-1)


def step(st, y, fault=None, reverse=False, extra=None):
    """One frame.  y complex64 [B, M, F] -> x complex128 [B, M, F]; ``extra``: a list of signals [B, M, F] that the same filter
    is applied to (returned as a list behind x).  ``fault``: one of FAULTS; ``reverse``: the other summation order."""
    M, taps, delay, G0 = st.M, st.taps, st.delay, st.G
    y32 = np.asarray(y).astype(np.complex64)
    yv = np.moveaxis(y32, 1, 2).astype(np.complex128)                           # [B, F, M]
    shift = 1 if fault == "z_late" else 0
    z = np.concatenate([st.ring[:, :, delay - 1 + k + shift, :] for k in range(taps)], axis=-1).astype(np.complex128)
    with np.errstate(all="ignore"):
        gz = np.conj(st.G) * z[..., :, None]
        if reverse:
            gz = gz[..., ::-1, :]
        x = yv - np.add.reduce(np.ascontiguousarray(gz), axis=-2)
        p = np.mean(yv.real ** 2 + yv.imag ** 2, axis=-1)                        # [B, F]
        cnt = min(int(st.n.flat[0]), st.context)
        if fault == "lambda_without_current":
            lam = st.pw[..., :cnt].sum(-1) / max(cnt, 1)
        else:
            lam = (p + st.pw[..., :cnt].sum(-1)) / (cnt + 1)
        lam = np.maximum(lam, st.power_floor)
        u = _matvec(st.P, z, reverse)
        zu = (z.real * u.real + z.imag * u.imag)
        zu = np.add.reduce(np.ascontiguousarray(zu[..., ::-1] if reverse else zu), axis=-1)
        d = st.alpha * lam + zu
        if fault == "float32_d":
            d = d.astype(np.float32).astype(np.float64)
        k = u / d[..., None]
        if fault == "k_zhp":                                                     # k (z^H P), no mirror: P drifts off Hermitian
            zhp = np.add.reduce(np.conj(z)[..., :, None] * st.P, axis=-2)
            Pn = st.P - k[..., :, None] * zhp[..., None, :]
        else:
            Pn = st.P - k[..., :, None] * np.conj(u)[..., None, :]
            low = np.tril(Pn)
            Pn = low + np.conj(np.swapaxes(np.tril(Pn, -1), -1, -2))
            i = np.arange(Pn.shape[-1])
            Pn[..., i, i] = Pn[..., i, i].real
        if fault != "p_not_divided":
            Pn = Pn / st.alpha
        Gn = st.G + k[..., :, None] * np.conj(yv if fault == "g_with_y" else x)[..., None, :]
    bad = ~np.isfinite(yv).all(-1) | ~(np.isfinite(d) & (d > 0))                # [B, F]
    ok = ~bad
    st.P = np.where(ok[..., None, None], Pn, st.P)
    st.G = np.where(ok[..., None, None], Gn, st.G)
    x = np.where(ok[..., None], x, yv)
    outs = None
    if extra is not None:
        if st.extra is None:
            st.extra = [np.zeros(st.ring.shape, np.complex128) for _ in extra]
        outs = []
        for r, e in zip(st.extra, extra):
            ev = np.moveaxis(np.asarray(e), 1, 2).astype(np.complex128)
            ze = np.concatenate([r[:, :, delay - 1 + kk, :] for kk in range(taps)], axis=-1)
            outs.append(np.moveaxis(ev - np.einsum("bfnm,bfn->bfm", np.conj(G0), ze), 2, 1))
            r[:, :, 1:] = r[:, :, :-1].copy()
            r[:, :, 0] = ev
    st.ring[:, :, 1:] = st.ring[:, :, :-1].copy()
    st.ring[:, :, 0] = np.where(ok[..., None], np.moveaxis(y32, 1, 2), 0)
    if st.context:
        st.pw[..., 1:] = st.pw[..., :-1].copy()
        st.pw[..., 0] = np.where(ok, p, 0.0)
    st.fail |= bad.astype(np.int32)
    st.n += 1
    xo = np.moveaxis(x, 2, 1)
    return xo if extra is None else (xo, outs)


def process(st, block, fault=None, reverse=False, extra=None):
    """block complex64 [B, M, T, F] -> complex64 of the same shape (with ``extra``: also the filtered companions, complex128)"""
    block = np.asarray(block)
    out = np.zeros(block.shape, np.complex64)
    eo = None if extra is None else [np.zeros(block.shape, np.complex128) for _ in extra]
    for t in range(block.shape[2]):
        if extra is None:
            out[:, :, t] = step(st, block[:, :, t], fault, reverse).astype(np.complex64)
        else:
            x, es = step(st, block[:, :, t], fault, reverse, [e[:, :, t] for e in extra])
            out[:, :, t] = x.astype(np.complex64)
            for o, e in zip(eo, es):
                o[:, :, t] = e
    return out if extra is None else (out, eo)


def owpe(mix, taps=10, delay=3, context=0, alpha=0.999, power_floor=1e-10, init=1.0, cuts=None, fault=None, reverse=False):
    """The one-shot call: reset, then the stream in one piece or in the pieces ``cuts`` (lengths; the rest follows).  Returns
    (out complex64 [B, M, T, F], State)."""
    mix = np.asarray(mix)
    B, M, T, F = mix.shape
    st = State(B, M, F, taps, delay, context, alpha, power_floor, init)
    out = np.zeros(mix.shape, np.complex64)
    for t0, t1 in pieces(T, cuts):
        out[:, :, t0:t1] = process(st, mix[:, :, t0:t1], fault, reverse)
    return out, st


def pieces(T, cuts):
    """the (start, end) of every call when a stream of T frames is cut into calls of the lengths ``cuts`` and then the rest"""
    edges, t = [], 0
    for c in (cuts or []):
        if t >= T:
            break
        c = min(int(c), T - t)
        if c > 0:
            edges.append((t, t + c))
            t += c
    if t < T:
        edges.append((t, T))
    return edges


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = float(np.linalg.norm(b.ravel()))
    return float(np.linalg.norm((a - b).ravel())) / (den if den > 0 else 1.0)


def figures(mix, **kw):
    """The reference of one case and its bars: (out, State, bar) with bar = max(100 x the rel-L2 by which the reversed summation
    order moves G and P, STATE_FLOOR) -- the rule of iva_ref.figures."""
    out, st = owpe(mix, **kw)
    _, sr = owpe(mix, reverse=True, **kw)
    own = max(rel(sr.G, st.G), rel(sr.P, st.P))
    return out, st, max(100.0 * own, STATE_FLOOR), own


def rejected(cand_out, cand, out, st, bar):
    """what the device tests assert, as one predicate: True when a candidate (output, State) misses any bar"""
    if not (np.array_equal(cand.fail, st.fail) and np.array_equal(cand.n, st.n)):
        return True
    herm = np.array_equal(cand.P, np.conj(np.swapaxes(cand.P, -1, -2)))
    return (not herm) or rel(cand_out, out) > OUT_BAR or rel(cand.G, st.G) > bar or rel(cand.P, st.P) > bar


def fixed_room(seed, T=1600, F=8, M=4, rev=12, noise=0.02, delay=3):
    """One enveloped source through filters of ``rev`` taps decaying as e^(-0.35 l), plus noise.  Returns (mix complex64
    [1, M, T, F], early, late complex128): early = the taps below ``delay``, late = the taps from ``delay`` on."""
    rng = np.random.default_rng(seed)

    def cn(*shape):
        return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)

    t = np.arange(T + rev)[:, None]
    f = np.arange(F)[None, :]
    src = cn(T + rev, F) * (np.abs(np.sin(0.05 * t + f)) + 0.05)
    h = cn(M, rev, F) * np.exp(-0.35 * np.arange(rev))[None, :, None]
    early = np.zeros((1, M, T, F), np.complex128)
    late = np.zeros((1, M, T, F), np.complex128)
    for l in range(rev):
        part = h[:, l][:, None, :] * src[None, rev - l:rev - l + T, :]
        (early if l < delay else late)[0] += part
    mix = early + late + noise * cn(1, M, T, F)
    return mix.astype(np.complex64), early, late


def late_over_early(early, late):
    """late energy over early energy in the frames [T/4, T/2) and [3T/4, T)"""
    T = early.shape[2]
    sel = np.r_[T // 4:T // 2, 3 * T // 4:T]
    return float(np.sum(np.abs(late[:, :, sel]) ** 2) / np.sum(np.abs(early[:, :, sel]) ** 2))
