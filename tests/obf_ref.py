"""Float64 NumPy restatement of the online beamformer of csrc/obf.hip (include/misonet.h, "online beamformer"),
vectorised over the cells (item, source, bin), with explicit loops for the Cholesky factor and the two triangular solves.  The
project's own definition in the family of estimate-driven beamformers with exponentially forgotten covariances (Souden, Benesty
& Affes 2010; Higuchi et al. 2017; Boeddeker et al. 2018); pb_bss, ESPnet, nara_wpe and pyroomacoustics were not available and
were not compared.

State per cell (b, s, f): Phi_s, Phi_n [M, M] Hermitian, w [M] (the filter of the last frame; never read), n, fail.  ``reset``:
Phi_s = 0, Phi_n = init I, w = 0, n = 0, fail = 0.  Per new frame, y the M samples of mix and x those of images[b, s]:

    0. a non-finite sample in y or x: fail |= 1, Phi_s, Phi_n and w stay, out = 0
    1. v = y - x ("residual") or v = y ("mix")
    2. Phi_s <- alpha Phi_s + (1 - alpha) x x^H, Phi_n <- alpha Phi_n + (1 - alpha) v v^H (lower triangle computed, the upper its
       mirror, the diagonal real)
    3. R = Phi_n + (diag_load tr(Phi_n) / M + epsi) I
    4. R = L L^H, column by column, inner sums over k ascending, 1 / L[c, c] formed once; a pivot not finite or not > 0:
       fail |= 2, w = 0, out = 0
    5. G = R^-1 Phi_s: L Z = Phi_s (k ascending), L^H G = Z (k descending); den = mu + sum_m G[m, m]; den not finite: fail |= 4,
       w = 0, out = 0; den == 0: w = 0, out = 0, no flag; else w = G[:, ref_ch] (1 / den), the reciprocal in Smith's form
    6. out = sum_m conj(w_m) y_m, rounded once to complex64
    7. n <- min(n + 1, 2^31 - 1)

The device tests compare against this file; ``FAULTS`` are the planted mistakes that tests/test_obf.py shows the device tests'
bars reject.
"""
import functools

import numpy as np

import iva_ref
import oiva_ref

OUT_BAR = 2.4e-7            # 4 x 2^-24: one complex64 rounding of a float64 result (the bar of oiva_ref and test_gpu_wpe.py)
STATE_FLOOR = 1e-12         # Phi_s, Phi_n and w: 100 x the restatement's own rounding figure on the case, never below this ...
BAR_CAP = 1e-6              # ... and a case whose bar would be above this is not a case
NOISES = ("residual", "mix")
FAULTS = ("phi_without_1_minus_alpha", "stale_covariances", "real_trace_phi_s", "no_conjugate", "load_not_over_m", "residual_is_y",
          "float32_phi")
N_MAX = 0x7FFFFFFF
pieces = oiva_ref.pieces
rel = oiva_ref.rel
hermitian = oiva_ref.hermitian


def _real(dtype):
    return np.empty(0, dtype).real.dtype


class State:
    """the state of B x S x F cells"""

    def __init__(self, B, S, M, F, noise="residual", ref_ch=0, alpha=0.98, mu=0.0, diag_load=1e-3, epsi=1e-10, init=1.0,
                 dtype=np.complex128):
        self.B, self.S, self.M, self.F = B, S, M, F
        self.noise = NOISES[noise] if isinstance(noise, (int, np.integer)) else noise
        self.ref_ch, self.alpha, self.mu, self.diag_load, self.epsi, self.init, self.dtype = ref_ch, alpha, mu, diag_load, epsi, init, dtype
        self.reset()

    def reset(self):
        B, S, M, F = self.B, self.S, self.M, self.F
        i = np.arange(M)
        self.phi_s = np.zeros((B, S, F, M, M), self.dtype)
        self.phi_n = np.zeros((B, S, F, M, M), self.dtype)
        self.phi_n[..., i, i] = self.init
        self.w = np.zeros((B, S, F, M), self.dtype)
        self.n = np.zeros((B, S, F), np.int32)
        self.fail = np.zeros((B, S, F), np.int32)


def _order(lo, hi, descending):
    """the integers lo .. hi - 1, ascending or descending"""
    return range(hi - 1, lo - 1, -1) if descending else range(lo, hi)


def smith_inv(p):
    """1 / p in Smith's form, part by part"""
    re, im = p.real, p.imag
    big = np.abs(re) >= np.abs(im)
    with np.errstate(all="ignore"):
        r1 = im / re
        d1 = re + im * r1
        r2 = re / im
        d2 = re * r2 + im
        out = np.empty(p.shape, p.dtype)
        out.real = np.where(big, 1.0 / d1, r2 / d2)
        out.imag = np.where(big, -r1 / d1, -1.0 / d2)
    return out


def cholesky(R, reverse=False):
    """R [..., M, M] -> (L [..., M, M] strictly lower, inv [..., M] = 1 / L[c, c], bad [...]): explicit loops, no pivoting"""
    M = R.shape[-1]
    rdt = _real(R.dtype)
    L = np.zeros_like(R)
    inv = np.zeros(R.shape[:-1], rdt)
    bad = np.zeros(R.shape[:-2], bool)
    for c in range(M):
        acc = R[..., :, c].copy()
        for k in _order(0, c, reverse):
            acc = acc - L[..., :, k] * np.conj(L[..., c, k])[..., None]
        p = acc[..., c].real
        bad |= ~(np.isfinite(p) & (p > 0))
        inv[..., c] = rdt.type(1.0) / np.sqrt(p)
        col = acc * inv[..., c, None]
        col[..., :c + 1] = 0
        L[..., :, c] = col
    return L, inv, bad


def solve(L, inv, rhs, reverse=False):
    """G = (L L^H)^-1 rhs by the two triangular solves, explicit loops; rhs [..., M, R]"""
    M = L.shape[-1]
    Z = np.zeros_like(rhs)
    for c in range(M):
        acc = rhs[..., c, :].copy()
        for k in _order(0, c, reverse):
            acc = acc - L[..., c, k, None] * Z[..., k, :]
        Z[..., c, :] = acc * inv[..., c, None]
    G = np.zeros_like(rhs)
    for c in range(M - 1, -1, -1):
        acc = Z[..., c, :].copy()
        for k in _order(c + 1, M, not reverse):
            acc = acc - np.conj(L[..., k, c, None]) * G[..., k, :]
        G[..., c, :] = acc * inv[..., c, None]
    return G


def _mirror(P):
    M = P.shape[-1]
    P = np.tril(P) + np.conj(np.swapaxes(np.tril(P, -1), -1, -2))
    i = np.arange(M)
    P[..., i, i] = P[..., i, i].real
    return P


def step(st, x, y, fault=None, reverse=False):
    """One frame.  x complex64 [B, S, M, F] (the images), y complex64 [B, M, F] (the mixture) -> out [B, S, F] in the State's dtype"""
    M, cdt = st.M, st.dtype
    rdt = _real(cdt)
    alpha, oma = rdt.type(st.alpha), rdt.type(1.0) - rdt.type(st.alpha)
    xv = np.moveaxis(np.asarray(x).astype(np.complex64), 2, 3).astype(cdt)                        # [B, S, F, M]
    yv = np.broadcast_to(np.moveaxis(np.asarray(y).astype(np.complex64), 1, 2).astype(cdt)[:, None], xv.shape)
    bad = ~(np.isfinite(xv.real) & np.isfinite(xv.imag) & np.isfinite(yv.real) & np.isfinite(yv.imag)).all(-1)   # [B, S, F]
    xv = np.where(bad[..., None], 0, xv)
    yv = np.where(bad[..., None], 0, yv)
    vv = yv - xv if (st.noise == "residual" and fault != "residual_is_y") else yv
    g = rdt.type(1.0) if fault == "phi_without_1_minus_alpha" else oma
    di = np.arange(M)
    with np.errstate(all="ignore"):
        new_s = _mirror(alpha * st.phi_s + g * (xv[..., :, None] * np.conj(xv[..., None, :])))
        new_n = _mirror(alpha * st.phi_n + g * (vv[..., :, None] * np.conj(vv[..., None, :])))
        if fault == "float32_phi":
            new_s, new_n = new_s.astype(np.complex64).astype(cdt), new_n.astype(np.complex64).astype(cdt)
        new_s = np.where(bad[..., None, None], st.phi_s, new_s)
        new_n = np.where(bad[..., None, None], st.phi_n, new_n)
        use_s, use_n = (st.phi_s, st.phi_n) if fault == "stale_covariances" else (new_s, new_n)
        diag = use_n[..., di, di].real
        tr = np.zeros(diag.shape[:-1], rdt)
        for m in _order(0, M, reverse):
            tr = tr + diag[..., m]
        load = rdt.type(st.diag_load) * tr / (rdt.type(1.0) if fault == "load_not_over_m" else rdt.type(M)) + rdt.type(st.epsi)
        R = use_n.copy()
        R[..., di, di] = R[..., di, di] + load[..., None]
        L, inv, pbad = cholesky(R, reverse)
        G = solve(L, inv, use_s, reverse)
        acc = np.zeros(G.shape[:-2], cdt)
        for m in _order(0, M, reverse):
            acc = acc + (use_s[..., m, m].real if fault == "real_trace_phi_s" else G[..., m, m])
        den = acc + rdt.type(st.mu)
        fin = np.isfinite(den.real) & np.isfinite(den.imag)
        zero = (den.real == 0) & (den.imag == 0)
        w = G[..., :, st.ref_ch] * smith_inv(den)[..., None]
        ok = ~bad & ~pbad & fin & ~zero
        w = np.where(ok[..., None], w, 0)
        terms = (w if fault == "no_conjugate" else np.conj(w)) * yv
        out = np.zeros(terms.shape[:-1], cdt)
        for m in _order(0, M, reverse):
            out = out + terms[..., m]
    st.phi_s, st.phi_n = new_s, new_n
    st.w = np.where(bad[..., None], st.w, w)
    st.fail |= (np.where(bad, 1, 0) | np.where(~bad & pbad, 2, 0) | np.where(~bad & ~pbad & ~fin, 4, 0)).astype(np.int32)
    st.n = np.minimum(st.n.astype(np.int64) + 1, N_MAX).astype(np.int32)
    return np.where(ok, out, 0)


def process(st, images, mix, fault=None, reverse=False):
    """images complex64 [B, S, M, T, F], mix complex64 [B, M, T, F] -> out complex64 [B, S, T, F]"""
    images, mix = np.asarray(images), np.asarray(mix)
    B, S, M, T, F = images.shape
    out = np.zeros((B, S, T, F), np.complex64)
    for t in range(T):
        out[:, :, t] = step(st, images[:, :, :, t], mix[:, :, t], fault, reverse).astype(np.complex64)
    return out


def obf(images, mix, cuts=None, fault=None, reverse=False, dtype=np.complex128, **opts):
    """The one-shot call: reset, then the stream in one piece or in the pieces ``cuts`` (lengths; the rest follows).  images
    complex64 [B, S, M, T, F], mix complex64 [B, M, T, F] -> (out complex64 [B, S, T, F], State)"""
    images, mix = np.asarray(images), np.asarray(mix)
    B, S, M, T, F = images.shape
    assert mix.shape == (B, M, T, F), (images.shape, mix.shape)
    st = State(B, S, M, F, dtype=dtype, **opts)
    out = np.zeros((B, S, T, F), np.complex64)
    for t0, t1 in pieces(T, cuts):
        out[:, :, t0:t1] = process(st, images[:, :, :, t0:t1], mix[:, :, t0:t1], fault, reverse)
    return out, st


def figures(images, mix, **kw):
    """The reference of one case and its bar: dict(out, st, ext, bar, own).  Phi_s, Phi_n and w are measured against the
    clongdouble run (``ext``); bar = max(100 x own, STATE_FLOOR), own = the larger of the rel-L2 distances float64 - clongdouble
    and float64 - reversed summation order on Phi_s, Phi_n and w: the rule of oiva_ref.figures."""
    out, st = obf(images, mix, **kw)
    _, ext = obf(images, mix, dtype=np.clongdouble, **kw)
    out_rev, rev = obf(images, mix, reverse=True, **kw)
    own = max(max(rel(getattr(st, k), getattr(o, k)) for k in ("phi_s", "phi_n", "w")) for o in (ext, rev))
    return dict(out=out, out_rev=out_rev, st=st, ext=ext, bar=max(100.0 * own, STATE_FLOOR), own=own)


def rejected(cand, ref):
    """what the device tests assert, as one predicate: True when a candidate dict(out, phi_s, phi_n, w, fail, n) misses any bar
    of the reference ``figures`` dict"""
    st, ext, bar = ref["st"], ref["ext"], ref["bar"]
    if not (np.array_equal(cand["fail"], st.fail) and np.array_equal(cand["n"], st.n)):
        return True
    if not (hermitian(cand["phi_s"]) and hermitian(cand["phi_n"])):
        return True
    return (rel(cand["out"], ref["out"]) > OUT_BAR or rel(cand["phi_s"], ext.phi_s) > bar or rel(cand["phi_n"], ext.phi_n) > bar
            or rel(cand["w"], ext.w) > bar)


def as_candidate(out, st):
    c128 = lambda a: a.astype(np.complex128)
    return dict(out=out, phi_s=c128(st.phi_s), phi_n=c128(st.phi_n), w=c128(st.w), fail=st.fail, n=st.n)


@functools.lru_cache(maxsize=None)
def inputs(B, S, M, T, F):
    """(images complex64 [B, S, M, T, F], mix complex64 [B, M, T, F]) of a case: M sources at M microphones in the stream layout,
    the images those of the restated online AuxIVA at alpha 0.96 (its first S rows).  Cached and read-only."""
    mix = oiva_ref.to_stream(iva_ref.sparse_mixture(B, M, M, T, F, seed=B + M + T + F)[0])
    images = np.ascontiguousarray(oiva_ref.oiva(mix, alpha=0.96)[1][:, :S])
    mix.setflags(write=False)
    images.setflags(write=False)
    return images, mix


def rank_one(M, T, F, seed, noise=0.3):
    """images = a (x) s_t with a fixed vector a per bin (every entry non-zero), mix = images + noise: (images [1, 1, M, T, F], mix
    [1, M, T, F], a [F, M]).  a is made of small integers and s of multiples of 1 / 64, so that the products a s_t are exact in
    complex64 and Phi_s is rank one up to float64 rounding"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(1, 4, (F, M)) * rng.choice([-1, 1], (F, M)) + 1j * rng.integers(-3, 4, (F, M))).astype(np.complex64)
    s = (np.round(64 * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))) / 64).astype(np.complex64)
    images = (a.T[:, None, :] * s[None]).astype(np.complex64)[None, None]            # [1, 1, M, T, F]
    assert np.array_equal(images[0, 0].astype(np.complex128), a.T[:, None, :].astype(np.complex128) * s[None].astype(np.complex128))
    nz = noise * (rng.standard_normal((1, M, T, F)) + 1j * rng.standard_normal((1, M, T, F)))
    return np.ascontiguousarray(images), np.ascontiguousarray((images[0] + nz).astype(np.complex64)), a
